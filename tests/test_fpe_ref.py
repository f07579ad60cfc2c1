"""The FPE reference itself (tests/xform_fpe_ref.py, no GPU): its AES against FIPS-197 appendix C.1 and C.3,
its FF1 against NIST's nine FF1 samples (three keys, an empty tweak and two tweaks, radix 10 and 36), decrypt
inverting each, and the transformation's literals."""
import pytest

import xform_fpe_ref as FR

PLAIN = bytes.fromhex("00112233445566778899aabbccddeeff")
A36 = "0123456789abcdefghijklmnopqrstuvwxyz"
SAMPLES = [
    (b"", 10, "0123456789", ("2433477484", "2830668132", "6657667009")),
    (bytes.fromhex("39383736353433323130"), 10, "0123456789", ("6124200773", "2496655549", "1001623463")),
    (bytes.fromhex("3737373770717273373737"), 36, "0123456789abcdefghi",
     ("a9tv40mll9kdu509eum", "xbj3kv35jrawxv32ysr", "xs8a0azh2avyalyzuwd")),
]


def test_aes_fips197_appendix_c():
    assert FR.aes_encrypt(bytes(range(16)), PLAIN).hex() == "69c4e0d86a7b0430d8cdb78070b4c55a"
    assert FR.aes_encrypt(bytes(range(32)), PLAIN).hex() == "8ea2b7ca516745bfeafc49904b496089"
    assert FR.SBOX[0] == 0x63 and FR.SBOX[0x53] == 0xED and sorted(FR.SBOX) == list(range(256))
    assert [len(FR.aes_round_keys(bytes(n))) for n in (16, 24, 32)] == [44, 52, 60]


@pytest.mark.parametrize("k", range(9))
def test_ff1_nist_samples(k):
    tweak, radix, plain, want = SAMPLES[k // 3]
    key = (FR.K128, FR.K192, FR.K256)[k % 3]
    x = [A36.index(c) for c in plain]
    y = FR.ff1_encrypt(key, radix, x, tweak)
    assert "".join(A36[d] for d in y) == want[k % 3]
    assert FR.ff1_decrypt(key, radix, y, tweak) == x


def test_empty_tweak_samples_are_the_constants():
    assert [FR.NIST_EMPTY[k].decode() for k in (FR.K128, FR.K192, FR.K256)] == list(SAMPLES[0][3])
    assert len(FR.K128) == 16 and len(FR.K192) == 24 and len(FR.K256) == 32


@pytest.mark.parametrize("k", range(len(FR.KNOWN)))
def test_literals(k):
    piece, name, key, want = FR.KNOWN[k]
    alphabet = FR.COMMON[name]
    assert FR.surrogate(key, alphabet, piece) == want and len(want) == len(piece)
    if FR.fallen_back(alphabet, piece):
        assert want == b"*" * len(piece)
    else:
        assert FR.surrogate(key, alphabet, want, decrypt=True) == piece
        want.decode("utf-8")


def test_limits():
    assert {r: FR.limits(r) for r in (2, 10, 16, 36, 62, 95)} == {
        2: (7, 64), 10: (2, 64), 16: (2, 64), 36: (2, 48), 62: (2, 42), 95: (2, 38)}
    assert len(FR.ALPHA95) == 95 == len(set(FR.ALPHA95))


class _F:
    def __init__(self, s, e, t):
        self.start, self.end, self.type_id = s, e, t


def test_apply_transform_mixes_the_kinds_and_decrypts():
    import xform_configs as X
    names = ["CREDIT_CARD_NUMBER", "EMAIL_ADDRESS", "SOCIAL_HANDLE", "IP_ADDRESS"]
    cfg = X.with_block(FR.F)
    text = b"card 4111 1111 1111 1111 mail jane.doe@corp.example.org @bob at 10.20.30.40."
    fs = [_F(5, 24, 0), _F(30, 55, 1), _F(56, 60, 2), _F(64, 75, 3)]
    assert [text[f.start:f.end] for f in fs] == [FR.CARD, b"jane.doe@corp.example.org", b"@bob", b"10.20.30.40"]
    out = FR.apply_transform(text, fs, names, cfg)
    mail = FR.surrogate(FR.KB, FR.COMMON["ALPHA_NUMERIC"], b"jane.doe@corp.example.org")
    assert out == b"card " + FR.CARD_KA + b" mail " + mail + b"  at [IP_ADDRESS]."
    # under the catch-all every row keeps its length and decrypts to itself
    cfc = X.with_block(FR.FC)
    enc = FR.apply_transform(text, fs, names, cfc)
    assert len(enc) == len(text) and enc != text
    assert FR.apply_transform(enc, fs, names, cfc, decrypt=True) == text
