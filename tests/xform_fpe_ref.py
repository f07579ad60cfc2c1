"""crypto_replace_ffx_fpe_config for the transformation tests: xform_hash_ref.apply_transform extended with
the FF1 surrogate (NIST SP 800-38G over AES, FIPS-197), both directions, in plain Python with big integers.
Written from the two standards and DESIGN section 4's definition; it shares no code with the compiler's key
expansion or the engine's cipher.  Also the two FPE configs the tests use (F, FC) and their keys.

The definition: a finding's bytes that belong to the alphabet, in order, are the numeral string (a numeral's
value is its character's position in the alphabet); every other byte stays where it is; the ciphertext
numerals go back into the same positions; the tweak is empty.  A finding with fewer than nmin or more than
nmax numerals is not encrypted: every one of its bytes becomes "*"."""
import base64
import functools
import string

import xform_hash_ref

KA = bytes(range(16))
KB = bytes(range(32))
KC = bytes(range(24))

COMMON = {"NUMERIC": string.digits, "HEXADECIMAL": string.digits + "ABCDEF",
          "UPPER_CASE_ALPHA_NUMERIC": string.digits + string.ascii_uppercase,
          "ALPHA_NUMERIC": string.digits + string.ascii_uppercase + string.ascii_lowercase}
# the 95 printable ASCII characters, in code order, and a 2-character alphabet
ALPHA95 = "".join(chr(c) for c in range(0x20, 0x7F))
ALPHA2 = "ab"


# ------------------------------------------------------------------------------------------------ AES
def _gmul(a: int, b: int) -> int:
    r = 0
    while b:
        if b & 1:
            r ^= a
        a = (a << 1) ^ (0x11B if a & 0x80 else 0)
        b >>= 1
    return r


def _make_sbox():
    inv = [0] * 256
    for a in range(1, 256):
        for b in range(1, 256):
            if _gmul(a, b) == 1:
                inv[a] = b
                break
    box = []
    for a in range(256):
        x = inv[a]
        y = x
        for _ in range(4):
            x = ((x << 1) | (x >> 7)) & 0xFF
            y ^= x
        box.append(y ^ 0x63)
    return box


SBOX = _make_sbox()


@functools.lru_cache(maxsize=None)
def _round_key_bytes(key: bytes):
    w = aes_round_keys(key)
    return [b"".join(x.to_bytes(4, "big") for x in w[4 * r:4 * r + 4]) for r in range(len(w) // 4)]


def aes_round_keys(key: bytes):
    """FIPS-197 5.2: 4 * (Nr + 1) words"""
    nk = len(key) // 4
    assert len(key) in (16, 24, 32)
    nr = nk + 6
    w = [int.from_bytes(key[4 * i:4 * i + 4], "big") for i in range(nk)]
    rcon = 1
    for i in range(nk, 4 * (nr + 1)):
        t = w[i - 1]
        if i % nk == 0:
            t = ((t << 8) | (t >> 24)) & 0xFFFFFFFF
            t = int.from_bytes(bytes(SBOX[b] for b in t.to_bytes(4, "big")), "big") ^ (rcon << 24)
            rcon = _gmul(rcon, 2)
        elif nk > 6 and i % nk == 4:
            t = int.from_bytes(bytes(SBOX[b] for b in t.to_bytes(4, "big")), "big")
        w.append(w[i - nk] ^ t)
    return w


def aes_encrypt(key: bytes, block: bytes) -> bytes:
    """FIPS-197 5.1, by the book: the state is 16 bytes, column-major (byte 4c + r = row r of column c)"""
    rk = _round_key_bytes(key)                 # (the schedule is the same for every block of a key)
    nr = len(rk) - 1

    def add(s, r):
        return [a ^ b for a, b in zip(s, rk[r])]
    s = add(list(block), 0)
    for r in range(1, nr + 1):
        s = [SBOX[b] for b in s]
        s = [s[4 * ((c + row) % 4) + row] for c in range(4) for row in range(4)]          # ShiftRows
        if r != nr:
            m = []
            for c in range(4):
                a = s[4 * c:4 * c + 4]
                m += [_gmul(a[i], 2) ^ _gmul(a[(i + 1) % 4], 3) ^ a[(i + 2) % 4] ^ a[(i + 3) % 4] for i in range(4)]
            s = m
        s = add(s, r)
    return bytes(s)


# ------------------------------------------------------------------------------------------------ FF1
def _num(digits, radix: int) -> int:
    x = 0
    for d in digits:
        x = x * radix + d
    return x


def _str(x: int, radix: int, m: int):
    out = [0] * m
    for i in range(m - 1, -1, -1):
        x, out[i] = divmod(x, radix)
    return out


def _ff1_setup(n: int, radix: int, tweak: bytes):
    u = n // 2
    v = n - u
    b = ((radix ** v - 1).bit_length() + 7) // 8
    d = 4 * ((b + 3) // 4) + 4
    p = bytes([1, 2, 1]) + radix.to_bytes(3, "big") + bytes([10, u % 256]) + n.to_bytes(4, "big") + \
        len(tweak).to_bytes(4, "big")
    return u, v, b, d, p


def _ff1_round(key, p, tweak, b, d, i, num_b):
    q = tweak + bytes((-len(tweak) - b - 1) % 16) + bytes([i]) + num_b.to_bytes(b, "big")
    y = bytes(16)
    pq = p + q
    for j in range(0, len(pq), 16):
        y = aes_encrypt(key, bytes(a ^ c for a, c in zip(y, pq[j:j + 16])))
    s = y
    j = 1
    while len(s) < d:
        s += aes_encrypt(key, bytes(a ^ c for a, c in zip(y, j.to_bytes(16, "big"))))
        j += 1
    return int.from_bytes(s[:d], "big")


def ff1_encrypt(key: bytes, radix: int, digits, tweak: bytes = b""):
    """SP 800-38G Algorithm 7; digits: a list of numerals"""
    n = len(digits)
    u, v, b, d, p = _ff1_setup(n, radix, tweak)
    A, B = list(digits[:u]), list(digits[u:])
    for i in range(10):
        y = _ff1_round(key, p, tweak, b, d, i, _num(B, radix))
        m = u if i % 2 == 0 else v
        c = (_num(A, radix) + y) % radix ** m
        A, B = B, _str(c, radix, m)
    return A + B


def ff1_decrypt(key: bytes, radix: int, digits, tweak: bytes = b""):
    """SP 800-38G Algorithm 8"""
    n = len(digits)
    u, v, b, d, p = _ff1_setup(n, radix, tweak)
    A, B = list(digits[:u]), list(digits[u:])
    for i in range(9, -1, -1):
        y = _ff1_round(key, p, tweak, b, d, i, _num(A, radix))
        m = u if i % 2 == 0 else v
        c = (_num(B, radix) - y) % radix ** m
        A, B = _str(c, radix, m), A
    return A + B


# ---------------------------------------------------------------------------------- the transformation
def limits(radix: int):
    """(nmin, nmax): the least n >= 2 with radix^n >= 100; min(2 * vmax, 64), radix^vmax <= 2^128"""
    nmin = 2
    while radix ** nmin < 100:
        nmin += 1
    vmax = 1
    while radix ** (vmax + 1) <= 1 << 128:
        vmax += 1
    return nmin, min(2 * vmax, 64)


def alphabet_of(fpe_cfg: dict) -> str:
    if "common_alphabet" in fpe_cfg:
        return COMMON[fpe_cfg["common_alphabet"]]
    return fpe_cfg["custom_alphabet"]


@functools.lru_cache(maxsize=None)
def surrogate(key: bytes, alphabet: str, piece: bytes, decrypt: bool = False) -> bytes:
    alpha = alphabet.encode("ascii")
    at = [i for i, c in enumerate(piece) if c in alpha]
    nmin, nmax = limits(len(alpha))
    if not nmin <= len(at) <= nmax:
        return b"*" * len(piece)
    ys = (ff1_decrypt if decrypt else ff1_encrypt)(key, len(alpha), [alpha.index(piece[i]) for i in at])
    out = bytearray(piece)
    for i, y in zip(at, ys):
        out[i] = alpha[y]
    return bytes(out)


def fallen_back(alphabet: str, piece: bytes) -> bool:
    n = sum(c in alphabet.encode("ascii") for c in piece)
    nmin, nmax = limits(len(alphabet))
    return not nmin <= n <= nmax


def fpe_prim(key: bytes, common: str = None, custom: str = None) -> dict:
    cfg = {"crypto_key": {"unwrapped": {"key": base64.b64encode(key).decode()}}}
    if common is not None:
        cfg["common_alphabet"] = common
    if custom is not None:
        cfg["custom_alphabet"] = custom
    return {"crypto_replace_ffx_fpe_config": cfg}


def _types(*names):
    return [{"name": n} for n in names]


# F: card, SSN and phone NUMERIC under KA, SWIFT and IBAN UPPER_CASE_ALPHA_NUMERIC under KC, e-mail
# ALPHA_NUMERIC under KB, handles removed, the rest "[TYPE]"
F = [
    {"info_types": _types("CREDIT_CARD_NUMBER", "US_SOCIAL_SECURITY_NUMBER", "PHONE_NUMBER"),
     "primitive_transformation": fpe_prim(KA, "NUMERIC")},
    {"info_types": _types("SWIFT_CODE", "IBAN_CODE"),
     "primitive_transformation": fpe_prim(KC, "UPPER_CASE_ALPHA_NUMERIC")},
    {"info_types": _types("EMAIL_ADDRESS"), "primitive_transformation": fpe_prim(KB, "ALPHA_NUMERIC")},
    {"info_types": _types("SOCIAL_HANDLE"), "primitive_transformation": {"redact_config": {}}},
    {"primitive_transformation": {"replace_with_info_type_config": {}}},
]
F_NUMERIC = ("CREDIT_CARD_NUMBER", "US_SOCIAL_SECURITY_NUMBER", "PHONE_NUMBER")
F_UPPER = ("SWIFT_CODE", "IBAN_CODE")
F_FPE = F_NUMERIC + F_UPPER + ("EMAIL_ADDRESS",)
# FC: one catch-all ALPHA_NUMERIC under KA
FC = [{"primitive_transformation": fpe_prim(KA, "ALPHA_NUMERIC")}]

# literal known answers, computed with an independent implementation: (finding, alphabet, key, output)
CARD = b"4111 1111 1111 1111"
SSN = b"536-22-1234"
KNOWN = [
    (CARD, "NUMERIC", KA, b"9329 9759 1240 5582"),
    (CARD, "NUMERIC", KB, b"3480 5050 4367 0686"),
    (SSN, "NUMERIC", KA, b"598-59-5178"),
    (b"212-555-0187", "NUMERIC", KB, b"588-669-2893"),
    (b"10.20.30.40", "NUMERIC", KA, b"60.57.27.21"),
    (b"jane.doe@corp.example.org", "ALPHA_NUMERIC", KA, b"29mg.NbJ@hdTC.vACRK0X.wtl"),
    (b"COBADEFFXXX", "UPPER_CASE_ALPHA_NUMERIC", KC, b"LR23Q5090HM"),
    (b"DEADBEEF-00ff", "HEXADECIMAL", KA, b"7CBC397C-BBff"),
    ("José Núñez".encode(), "ALPHA_NUMERIC", KA, "DyGé yúñZ5".encode()),
    (b"a1b", "NUMERIC", KA, b"***"),
]
CARD_KA = KNOWN[0][3]
SSN_KA = KNOWN[2][3]

# NIST's FF1 samples
K128 = bytes.fromhex("2B7E151628AED2A6ABF7158809CF4F3C")
K192 = K128 + bytes.fromhex("EF4359D8D580AA4F")
K256 = K192 + bytes.fromhex("7F036D6F04FC6A94")
NIST_DIGITS = b"0123456789"
NIST_EMPTY = {K128: b"2433477484", K192: b"2830668132", K256: b"6657667009"}


def fpe_of(prim):
    return prim.get("crypto_replace_ffx_fpe_config") if prim is not None else None


def apply_transform(text: bytes, findings, names, config: dict, decrypt: bool = False) -> bytes:
    """xform_hash_ref.apply_transform, with crypto_replace_ffx_fpe_config.  findings: start / end / type_id,
    in order.  decrypt: the FPE findings are decrypted instead (text is then an FPE output; the spans of an
    FPE output are those of its input)"""
    import xform_ref
    out, pos = [], 0
    for f in findings:
        fpe = fpe_of(xform_ref.pick(names[f.type_id], config))
        if fpe is not None:
            key = base64.b64decode(fpe["crypto_key"]["unwrapped"]["key"])
            out.append(text[pos:f.start])
            out.append(surrogate(key, alphabet_of(fpe), text[f.start:f.end], decrypt))
        else:                    # every other kind: the existing reference, on this finding alone
            out.append(xform_hash_ref.apply_transform(text[pos:f.end], [xform_hash_ref._Shift(f, pos)], names, config))
        pos = f.end
    out.append(text[pos:])
    return b"".join(out)
