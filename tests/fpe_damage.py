"""Damage to the FPE sections of a compiled blob (xf.fpe, xf.fpe_key, xf.fpe_alpha), one defect each, with the
message the host rule preparation gives it: shared by test_fpe_host (the stand-alone program) and
test_gpu_fpe (pii_engine_create).  Each function edits the section dict of compiler.blob_sections in
place.  The blob is config F's (xform_fpe_ref.F): three keys, three alphabets."""
import numpy as np

KEY_WORDS, ALPHA_WORDS = 64, 68
NOT_ALL = "FPE sections are not all present"
INVERSE = "xf.fpe_alpha holds maps that are not inverse"
LIMITS = "xf.fpe_alpha holds numeral limits out of range"
LENGTHS = "xf.fpe_alpha holds byte lengths that are not ascending up to 16"


def _dropped(name):
    def f(S):
        del S[name]
    f.__name__ = "dropped_" + name.replace(".", "_")
    return f


def _fpe_type(S):
    return int(np.flatnonzero(S["xf.kind"] == 6)[0])


def _type_table_short(S):
    S["xf.fpe"] = S["xf.fpe"][:-1].copy()


def _key_record_cut(S):
    S["xf.fpe_key"] = S["xf.fpe_key"][:-1].copy()


def _key_table_empty(S):
    S["xf.fpe_key"] = S["xf.fpe_key"][:0].copy()


def _alphabet_record_cut(S):
    S["xf.fpe_alpha"] = S["xf.fpe_alpha"][:-4].copy()


def _seventeen_keys(S):
    S["xf.fpe_key"] = np.tile(S["xf.fpe_key"][:KEY_WORDS], 17)


def _key_past_the_table(S):
    w = S["xf.fpe"].copy()
    t = _fpe_type(S)
    w[t] = (w[t] & 0xFFFF0000) | (len(S["xf.fpe_key"]) // KEY_WORDS)
    S["xf.fpe"] = w


def _alphabet_past_the_table(S):
    w = S["xf.fpe"].copy()
    t = _fpe_type(S)
    w[t] = (w[t] & 0xFFFF) | (len(S["xf.fpe_alpha"]) // ALPHA_WORDS) << 16
    S["xf.fpe"] = w


def _rounds(nr, rec=1):
    def f(S):
        k = S["xf.fpe_key"].copy()
        k[rec * KEY_WORDS] = nr
        S["xf.fpe_key"] = k
    f.__name__ = "rounds_%d" % nr
    return f


def _record(S, radix):
    """the alphabet record of that radix (F: 10 NUMERIC, 36 UPPER_CASE_ALPHA_NUMERIC, 62 ALPHA_NUMERIC)"""
    return int(np.flatnonzero(S["xf.fpe_alpha"][::ALPHA_WORDS] == radix)[0])


def _alpha_word(i, v, radix=10):
    def f(S):
        rec = _record(S, radix)
        a = S["xf.fpe_alpha"].copy()
        a[rec * ALPHA_WORDS + i] = v
        S["xf.fpe_alpha"] = a
    f.__name__ = "alpha_word%d_%d" % (i, v)
    return f


def _alpha_byte(at, v, radix=62, name=None):
    """byte `at` of the record: 16.. the byte -> digit map, 144.. the digit -> byte map, 240.. b(v)"""
    def f(S):
        rec = _record(S, radix)
        a = S["xf.fpe_alpha"].astype("<u4")
        raw = a.view(np.uint8)
        raw[4 * rec * ALPHA_WORDS + at] = v(raw[4 * rec * ALPHA_WORDS:]) if callable(v) else v
        S["xf.fpe_alpha"] = a.astype(np.uint32)
    f.__name__ = name or "alpha_byte%d" % at
    return f


def _unknown_kind(S):
    k = S["xf.kind"].copy()
    k[_fpe_type(S)] = 7
    S["xf.kind"] = k


DAMAGE = [(_dropped(s), NOT_ALL) for s in ("xf.fpe", "xf.fpe_key", "xf.fpe_alpha")] + [
    (_type_table_short, "xf.fpe does not hold one word per type"),
    (_key_record_cut, "xf.fpe_key does not hold whole key records"),
    (_key_table_empty, "xf.fpe_key does not hold whole key records"),
    (_alphabet_record_cut, "xf.fpe_alpha does not hold whole alphabet records"),
    (_seventeen_keys, "xf.fpe_key holds too many keys"),
    (_key_past_the_table, "xf.fpe names a key past the key table"),
    (_alphabet_past_the_table, "xf.fpe names an alphabet past the alphabet table"),
    (_rounds(11), "xf.fpe_key holds a round count that is not 10, 12 or 14"),
    (_rounds(0), "xf.fpe_key holds a round count that is not 10, 12 or 14"),
    (_rounds(16), "xf.fpe_key holds a round count that is not 10, 12 or 14"),
    (_alpha_word(0, 1), "xf.fpe_alpha holds a radix outside 2..95"),
    (_alpha_word(0, 96), "xf.fpe_alpha holds a radix outside 2..95"),
    # a radix one larger or smaller than the maps hold
    (_alpha_word(0, 11), INVERSE),
    (_alpha_word(0, 9), INVERSE),
    # ALPHA_NUMERIC: 'A' -> the digit of 'B'; '#' -> digit 0; digit 1 -> a byte >= 0x80; 'A' -> digit 200
    (_alpha_byte(16 + 65, lambda r: r[16 + 66], name="two_bytes_one_digit"), INVERSE),
    (_alpha_byte(16 + 35, 0, name="byte_outside_mapped"), INVERSE),
    (_alpha_byte(144 + 1, 0xC3, name="digit_to_a_high_byte"), INVERSE),
    (_alpha_byte(16 + 65, 200, name="digit_past_the_radix"), INVERSE),
    (_alpha_word(1, 1), LIMITS),
    (_alpha_word(1, 65), LIMITS),
    (_alpha_word(2, 65), LIMITS),
    (_alpha_word(2, 1), LIMITS),
    (_alpha_byte(240 + 5, 17, name="length_17"), LENGTHS),
    (_alpha_byte(240, 0, name="length_0"), LENGTHS),
    (_alpha_byte(240 + 9, 1, name="length_descending"), LENGTHS),
    (_unknown_kind, "transformation tables malformed"),
]
IDS = ["%02d_%s" % (i, d.__name__.strip("_")) for i, (d, _) in enumerate(DAMAGE)]
