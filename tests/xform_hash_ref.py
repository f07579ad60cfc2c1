"""crypto_hash_config for the transformation tests: xform_ref.apply_transform extended with the
surrogate base64(HMAC-SHA256(key, finding bytes)), computed with the standard library's hmac / hashlib.
Written from DLP's description of the primitive; it shares no code with the compiler's SHA-256.  Also
the two hash configs the tests use (H, HC) and their keys."""
import base64
import hashlib
import hmac

import xform_ref

KEY1 = bytes(range(32))
KEY2 = bytes(range(64))
HASH_LEN = 44
PLACEHOLDER = b"=" * HASH_LEN


def hash_prim(key: bytes) -> dict:
    return {"crypto_hash_config": {"crypto_key": {"unwrapped": {"key": base64.b64encode(key).decode()}}}}


def _types(*names):
    return [{"name": n} for n in names]


# H: card, SSN and e-mail hashed under key 1, phone under key 2, handles removed, the rest "[TYPE]"
H = [
    {"info_types": _types("CREDIT_CARD_NUMBER", "US_SOCIAL_SECURITY_NUMBER", "EMAIL_ADDRESS"),
     "primitive_transformation": hash_prim(KEY1)},
    {"info_types": _types("PHONE_NUMBER"), "primitive_transformation": hash_prim(KEY2)},
    {"info_types": _types("SOCIAL_HANDLE"), "primitive_transformation": {"redact_config": {}}},
    {"primitive_transformation": {"replace_with_info_type_config": {}}},
]
H_HASHED = ("CREDIT_CARD_NUMBER", "US_SOCIAL_SECURITY_NUMBER", "EMAIL_ADDRESS", "PHONE_NUMBER")
# HC: one catch-all hash
HC = [{"primitive_transformation": hash_prim(KEY1)}]

# literal known answers (base64 of HMAC-SHA256), not computed here
CARD = b"4111 1111 1111 1111"
SSN = b"536-22-1234"
CARD_KEY1 = b"jrMNkIXGrig+48XipOe/98mj17+VHT1phtrs7Oed80A="
SSN_KEY1 = b"Hi7a/ma27PV5oGzlo6NUjZ667o4XmGchAnlBwu5CRR4="
SSN_KEY2 = b"eo3Ki9TEC7pjeGOr+7e9weEcDT8zJkC5PQ+9v1pp1kg="
JOSE_KEY1 = b"hR7tJpyEm3iAB09Kyx7dEUTeiDYZVvmcDNSuxg57B2w="       # "José Núñez" (UTF-8)


def surrogate(key: bytes, piece: bytes) -> bytes:
    return base64.b64encode(hmac.new(key, piece, hashlib.sha256).digest())


def apply_transform(text: bytes, findings, names, config: dict) -> bytes:
    """xform_ref.apply_transform, with crypto_hash_config.  findings: start / end / type_id, in order"""
    out, pos = [], 0
    for f in findings:
        prim = xform_ref.pick(names[f.type_id], config)
        if prim is not None and "crypto_hash_config" in prim:
            key = base64.b64decode(prim["crypto_hash_config"]["crypto_key"]["unwrapped"]["key"])
            out.append(text[pos:f.start])
            out.append(surrogate(key, text[f.start:f.end]))
        else:                    # every other kind: the existing reference, on this finding alone
            out.append(xform_ref.apply_transform(text[pos:f.end], [_Shift(f, pos)], names, config))
        pos = f.end
    out.append(text[pos:])
    return b"".join(out)


class _Shift:
    """a finding, relative to `pos`"""

    def __init__(self, f, pos):
        self.start, self.end, self.type_id = f.start - pos, f.end - pos, f.type_id
