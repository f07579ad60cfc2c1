"""Re-identification (pii_reidentify) in plain Python, on top of xform_fpe_ref: the definition the engine's
call is tested against.

The inputs are a de-identified row and the findings the de-identify call returned for it, in the coordinates of
that call's INPUT, in order.  Finding k was written at start_k + D_k, D_k = the sum over the earlier findings j
of out_len_j - (end_j - start_j), and is out_len_k bytes long: the finding's own length under
character_mask_config, crypto_replace_ffx_fpe_config and for a type no transformation names; the length of
"[NAME]" or of the replace_config string; 0 under redact_config; 44 under crypto_hash_config.  A finding under
crypto_replace_ffx_fpe_config is decrypted there with FF1 (xform_fpe_ref.ff1_decrypt over its bytes of the
alphabet); every other byte of the row stays.

Out of range: a range whose count of alphabet bytes is below nmin or above nmax is left as it is -- the
fail-closed "***" of the de-identify direction stays "***".  (xform_fpe_ref.surrogate(..., decrypt=True) returns
stars there; a re-identify never destroys text, so this module does not use that branch.)"""
import base64

import xform_fpe_ref as FR
import xform_hash_ref
import xform_ref


def out_len(type_name: str, n: int, config: dict) -> int:
    """bytes a finding of n bytes occupies in the de-identified row"""
    prim = xform_ref.pick(type_name, config)
    if prim is None or "character_mask_config" in prim or "crypto_replace_ffx_fpe_config" in prim:
        return n
    if "replace_with_info_type_config" in prim:
        return len(type_name.encode()) + 2
    if "replace_config" in prim:
        return len(prim["replace_config"]["new_value"]["string_value"].encode("utf-8"))
    if "crypto_hash_config" in prim:
        return xform_hash_ref.HASH_LEN
    assert "redact_config" in prim, prim
    return 0


def positions(findings, names, config: dict):
    """[(lo, hi)]: each finding's range in the de-identified row"""
    out, d = [], 0
    for f in findings:
        n = f.end - f.start
        m = out_len(names[f.type_id], n, config)
        out.append((f.start + d, f.start + d + m))
        d += m - n
    return out


def decrypt_piece(key: bytes, alphabet: str, piece: bytes) -> bytes:
    if FR.fallen_back(alphabet, piece):
        return piece
    return FR.surrogate(key, alphabet, piece, decrypt=True)


def reidentify(text: bytes, findings, names, config: dict) -> bytes:
    out = bytearray(text)
    for f, (lo, hi) in zip(findings, positions(findings, names, config)):
        assert 0 <= lo <= hi <= len(text), (lo, hi, len(text))
        fpe = FR.fpe_of(xform_ref.pick(names[f.type_id], config))
        if fpe is not None:
            key = base64.b64decode(fpe["crypto_key"]["unwrapped"]["key"])
            out[lo:hi] = decrypt_piece(key, FR.alphabet_of(fpe), text[lo:hi])
    return bytes(out)


class Finding:
    """a finding by hand: start / end / type_id"""

    def __init__(self, start, end, type_id):
        self.start, self.end, self.type_id = start, end, type_id
