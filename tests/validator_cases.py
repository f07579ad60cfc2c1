"""Inputs that pin the validators (csrc/pii_device.h: v_digits, v_luhn ... v_iban, RegSrc / MemSrc) to
oracle.VALIDATORS: exhaustive over the two lookup tables, every boundary of the range checks, and the same
digits in matches of at most 32 bytes (RegSrc, v_digits) and of more (MemSrc, the stand-alone validators).

Plain Python, no GPU, no synth.py: every generator returns (label, row) with row = b"x " + value + b" y", so
"\\b" holds on both sides of the value and nothing else in the row can match; random filler comes from
random.Random with a fixed seed.  No row holds a hotword and the configs built here have no rule sets.

Two rule files are built from here (builtin_short / builtin_long + dlp_config):
  short  the shipped patterns of the nine validated detectors, every likelihood LIKELY, nothing else -- a value
         its validator rejects gives no finding at all
  long   five detectors whose patterns exceed 32 bytes: LUHN_LONG, NANP_LONG, SSN_LONG, EIN_LONG, IPV4_LONG.
         Their separators differ ('-' ' ', '/', ':', ',') so that one detector's cases are not another's matches.
"""
import random

import yaml

LETTERS = "ABCDEFGHIJKLMNOPQRSTUVWXYZ"
DIGITS = "0123456789"
ALNUM = DIGITS + LETTERS

# validator -> the detector types that carry it, per rule file
SHORT_TYPES = {"nanp": ["PHONE_NUMBER"], "luhn": ["CREDIT_CARD_NUMBER", "IMEI_HARDWARE_ID"],
               "ssn": ["US_SOCIAL_SECURITY_NUMBER"], "ein": ["US_EMPLOYER_IDENTIFICATION_NUMBER"],
               "ipv4": ["IP_ADDRESS"], "swift": ["SWIFT_CODE"], "iban": ["IBAN_CODE"]}
LONG_DETECTORS = {
    "LUHN_LONG": {"pattern": r"\b\d(?:[- ]?\d){1,59}\b", "validator": "luhn", "likelihood": "LIKELY"},
    "NANP_LONG": {"pattern": r"\b\d(?:/{1,30}\d){9}\b", "validator": "nanp", "likelihood": "LIKELY"},
    "SSN_LONG": {"pattern": r"\b\d(?::{1,30}\d){8}\b", "validator": "ssn", "likelihood": "LIKELY"},
    "EIN_LONG": {"pattern": r"\b\d(?:,{1,30}\d){8}\b", "validator": "ein", "likelihood": "LIKELY"},
    "IPV4_LONG": {"pattern": r"[0-9.]{3,48}", "validator": "ipv4", "likelihood": "LIKELY"},
}
LONG_TYPES = {d["validator"]: [name] for name, d in LONG_DETECTORS.items()}
KINDS = ["luhn", "nanp", "ssn", "ein", "ipv4", "swift", "iban"]


def builtin_short(shipped: dict) -> dict:
    """the shipped detectors that have a validator, their patterns untouched, all LIKELY"""
    dets = {}
    for name, variants in shipped["detectors"].items():
        keep = [dict(v, likelihood="LIKELY") for v in variants if v.get("validator")]
        if keep:
            dets[name] = keep
    return {"likelihood_scale": shipped["likelihood_scale"], "detectors": dets}


def builtin_long(shipped: dict) -> dict:
    return {"likelihood_scale": shipped["likelihood_scale"],
            "detectors": {name: [dict(d)] for name, d in LONG_DETECTORS.items()}}


def dlp_config(builtin: dict) -> dict:
    """every type of the rule file listed, no rule sets, the default min_likelihood"""
    return {"inspect_config": {"info_types": [{"name": n} for n in builtin["detectors"]]}}


def write_rules(tmp_dir, name: str, builtin: dict):
    """(dlp_config path, builtin path) of one rule file pair written into tmp_dir"""
    import json
    import os
    cfg_path = os.path.join(str(tmp_dir), name + "_dlp_config.json")
    builtin_path = os.path.join(str(tmp_dir), name + "_builtin.yaml")
    with open(cfg_path, "w") as f:
        json.dump(dlp_config(builtin), f)
    with open(builtin_path, "w") as f:
        yaml.safe_dump(builtin, f)
    return cfg_path, builtin_path


def embed(value: bytes) -> bytes:
    return b"x " + value + b" y"


def value_of(row: bytes) -> bytes:
    return row[2:-2]


def _rows(pairs):
    return [(label, embed(v.encode() if isinstance(v, str) else v)) for label, v in pairs]


def _digits(rnd, n):
    return "".join(rnd.choice(DIGITS) for _ in range(n))


# ---------------------------------------------------------------------------------------- short forms
def swift():
    out = []
    for form, tail in (("8", "2L"), ("11", "2LXXX")):
        for a in LETTERS:
            for b in LETTERS:
                out.append(("swift/%s/%s%s" % (form, a, b), "BANK" + a + b + tail))
        # A / Z (and 0 / 9 where the pattern takes a digit) at every other position, under a listed and an
        # unlisted country
        n = 8 if form == "8" else 11
        for cc in ("DE", "DQ"):
            for p in [0, 1, 2, 3] + list(range(6, n)):
                for ch in "AZ" + ("09" if p >= 6 else ""):
                    v = list("MMMM" + cc + "M" * (n - 6))
                    v[p] = ch
                    out.append(("swift/%s/edge/%s/%d%s" % (form, cc, p, ch), "".join(v)))
    return _rows(out)


def ein():
    rnd = random.Random(41)
    return _rows(("ein/%02d" % p, "%02d-%s" % (p, _digits(rnd, 7))) for p in range(100))


SSN_AREAS = ["000", "001", "665", "666", "667", "899", "900", "999"]
SSN_GROUPS = ["00", "01", "99"]
SSN_SERIALS = ["0000", "0001", "9999"]


def _ssn_digits():
    return [(a, g, s) for a in SSN_AREAS for g in SSN_GROUPS for s in SSN_SERIALS]


def ssn():
    return _rows(("ssn/%s-%s-%s" % t, "%s-%s-%s" % t) for t in _ssn_digits())


def _nanp_digits():
    return [(d0, d3, "%d12" % d0, "%d55" % d3, "0187") for d0 in range(10) for d3 in range(10)]


def nanp():
    out = []
    for d0, d3, a, b, c in _nanp_digits():
        for form, v in (("dash", "%s-%s-%s" % (a, b, c)), ("dot", "%s.%s.%s" % (a, b, c)),
                        ("space", "%s %s %s" % (a, b, c)), ("paren", "(%s) %s-%s" % (a, b, c)),
                        ("bare", a + b + c)):
            out.append(("nanp/%s/%d%d" % (form, d0, d3), v))
    return _rows(out)


IPV4_FIELDS = ["0", "00", "000", "1", "9", "10", "99", "100", "199", "200", "249", "250", "255", "256", "260",
               "299", "300", "999"]


def ipv4():
    out = []
    for pos in range(4):
        for val in IPV4_FIELDS:
            f = ["10", "20", "30", "40"]
            f[pos] = val
            out.append(("ipv4/field%d/%s" % (pos, val), ".".join(f)))
    out.append(("ipv4/all255", "255.255.255.255"))
    out.append(("ipv4/all0", "0.0.0.0"))
    return _rows(out)


def _group(digits, sizes, sep):
    parts, i = [], 0
    for k in sizes:
        parts.append(digits[i:i + k])
        i += k
    assert i == len(digits)
    return sep.join(parts)


LUHN_FORMS = [("bare%d" % n, n, (lambda d: d)) for n in range(13, 20)] + [
    ("4444dash", 16, lambda d: _group(d, (4, 4, 4, 4), "-")),
    ("4444space", 16, lambda d: _group(d, (4, 4, 4, 4), " ")),
    ("465dash", 15, lambda d: _group(d, (4, 6, 5), "-")),
    ("465space", 15, lambda d: _group(d, (4, 6, 5), " ")),
    ("imei2661", 15, lambda d: _group(d, (2, 6, 6, 1), "-")),
]


def _luhn_tens(prefix, forms, rnd):
    """per form one random body with all ten final digits, and the same body with all ten first digits"""
    out = []
    for name, n, shape in forms:
        body = _digits(rnd, n)
        for d in DIGITS:
            out.append(("%s/%s/last/%s" % (prefix, name, d), shape(body[:-1] + d)))
        for d in DIGITS:
            out.append(("%s/%s/first/%s" % (prefix, name, d), shape(d + body[1:])))
    return out


def luhn():
    return _rows(_luhn_tens("luhn", LUHN_FORMS, random.Random(43)))


IBAN_LENGTHS = list(range(12, 36))           # what the shipped pattern can produce, unspaced
IBAN_CHECKS = ["%02d" % c for c in range(100)]    # 02..98, and 00, 01, 99
IBAN_COUNTRIES = ["DE", "GB", "AA", "AZ", "ZA", "ZZ"]


def iban_bbans(length: int):
    """two BBANs of length - 4 characters: digits and letters mixed around a run of 'Z', and 'Z' only"""
    rnd = random.Random(4700 + length)
    n = length - 4
    run = min(n, 7)
    mixed = [rnd.choice(ALNUM) for _ in range(n)]
    at = rnd.randrange(n - run + 1)
    mixed[at:at + run] = "Z" * run
    return [("mixed", "".join(mixed)), ("zrun", "Z" * n)]


def iban_spaced(v: str) -> str:
    return " ".join(v[i:i + 4] for i in range(0, len(v), 4))


def iban_values():
    """(label, unspaced value): per length and BBAN all hundred check values; at three lengths the other
    countries' letters too"""
    out = []
    for length in IBAN_LENGTHS:
        for k, (bname, bban) in enumerate(iban_bbans(length)):
            ccs = [IBAN_COUNTRIES[(length + k) % len(IBAN_COUNTRIES)]]
            if length in (15, 22, 34) and k == 0:
                ccs = IBAN_COUNTRIES
            for cc in ccs:
                for chk in IBAN_CHECKS:
                    out.append(("%d/%s/%s%s" % (length, bname, cc, chk), cc + chk + bban))
    return out


def iban():
    out = []
    for label, v in iban_values():
        out.append(("iban/plain/" + label, v))
        out.append(("iban/spaced/" + label, iban_spaced(v)))
    return _rows(out)


def iban_running_max(value: bytes) -> int:
    """the largest tail * m + v the device's recurrence (v_iban) forms before it reduces: characters 5 and
    later, 'tail' reduced modulo 97 once it reaches 1 << 24"""
    tail, top, length = 0, 0, 0
    for c in value:
        if c == 32:
            continue
        if 48 <= c <= 57:
            v, m = c - 48, 10
        else:
            v, m = c - 55, 100
        if length >= 4:
            t = tail * m + v
            top = max(top, t)
            tail = t % 97 if t >= 1 << 24 else t
        length += 1
    return top


# ----------------------------------------------------------------------------------------- long forms
LUHN_LONG_COUNTS = [2, 3, 12, 13, 16, 17, 18, 19, 20, 31, 32, 33, 34, 47, 48, 59, 60]


def _alternate(d):
    return "".join(c + ("- "[i & 1] if i + 1 < len(d) else "") for i, c in enumerate(d))


def luhn_long():
    """2 .. 60 digits bare (n = count) and with a separator after every digit (n = 2 * count - 1): 17, 18 and
    19 digits come in 32 bytes or fewer and in more"""
    forms = []
    for n in LUHN_LONG_COUNTS:
        forms.append(("bare%d" % n, n, lambda d: d))
        forms.append(("sep%d" % n, n, _alternate))
    return _rows(_luhn_tens("luhn_long", forms, random.Random(47)))


def _spread(digits: str, sep: str, gaps):
    assert len(gaps) == len(digits) - 1
    return "".join(c + (sep * gaps[i] if i < len(gaps) else "") for i, c in enumerate(digits))


def _widths(n_digits):
    """separator counts per gap: one or two each (32 bytes or fewer), three each (more than 32), 30 in the
    fourth gap"""
    g = n_digits - 1
    wide = [1] * g
    wide[3] = 30
    return [("w1", [1] * g), ("w2", [2] * g), ("w3", [3] * g), ("w30", wide)]


def nanp_long():
    out = []
    for d0, d3, a, b, c in _nanp_digits():
        for w, gaps in _widths(10):
            out.append(("nanp_long/%s/%d%d" % (w, d0, d3), _spread(a + b + c, "/", gaps)))
    return _rows(out)


def ssn_long():
    out = []
    for t in _ssn_digits():
        for w, gaps in _widths(9):
            out.append(("ssn_long/%s/%s-%s-%s" % ((w,) + t), _spread("".join(t), ":", gaps)))
    return _rows(out)


def ein_long():
    rnd = random.Random(53)
    out = []
    for p in range(100):
        body = _digits(rnd, 7)
        for w, gaps in _widths(9):
            out.append(("ein_long/%s/%02d" % (w, p), _spread("%02d%s" % (p, body), ",", gaps)))
    return _rows(out)


IPV4_SHAPES = ["1..2.3", "1.2..3", "..1.2", "...", ".1.2.3.4", "1.2.3.4.", "1.2.3.", "1.2.3", "1.2", "123",
               "1.2.3.4.5", "1.2.3.4", "1234.1.1.1", "1.1.1.1234", "0255.1.1.1", "1.1.1.0001", "0000.0.0.0",
               "4294967296.1.1.1", "1.1.1.4294967296", "1.4294967296.1.1", "4294967551.1.1.1",
               "1.1.1.4294967551", "1.1.4294967551.1", "255.255.255.255", "256.255.255.255", "0.0.0.0",
               "000.000.000.000", "99999999999999999999.1.1.1"]


def ipv4_long():
    """the loose pattern: the shipped boundaries again (15 bytes or fewer), the branches only it reaches, and the
    boundary values at the end of matches of more than 32 bytes -- four fields of which the first is too long,
    and fifteen fields.  (Four fields of at most three digits are at most 15 bytes: nothing longer is accepted.)"""
    out = [("ipv4_long/" + label[5:], value_of(row).decode()) for label, row in ipv4()]
    out += [("ipv4_long/shape/" + s, s) for s in IPV4_SHAPES]
    for val in IPV4_FIELDS:
        out.append(("ipv4_long/wide4/" + val, "0" * 24 + "1.2.3." + val))
        out.append(("ipv4_long/wide15/" + val, "1.2.3.4.5.6.7.8.9.10.11.12.13.14." + val))
        out.append(("ipv4_long/mid4/" + val, "0" * 8 + "1.2.3." + val))
    return _rows(out)


SHORT_CASES = {"luhn": luhn, "nanp": nanp, "ssn": ssn, "ein": ein, "ipv4": ipv4, "swift": swift, "iban": iban}
LONG_CASES = {"luhn": luhn_long, "nanp": nanp_long, "ssn": ssn_long, "ein": ein_long, "ipv4": ipv4_long}


def width_class(n: int) -> str:
    return "16" if n <= 16 else "32" if n <= 32 else "33+"


# a width class in which a validator accepts nothing, and why (every other class a validator's cases reach
# holds an accepted and a rejected case)
NEVER_ACCEPTED = {
    ("ipv4", "32"): "four fields of at most three digits are at most 15 bytes",
    ("ipv4", "33+"): "four fields of at most three digits are at most 15 bytes",
}


# -------------------------------------------------------------------------------- alignment families
def _oracle_validators():
    from oracle import pii_oracle as O
    return O.VALIDATORS


def _pick(kind, make, choices):
    """(accepted, rejected) among make(c) for c in choices, under the oracle"""
    V = _oracle_validators()[kind]
    acc = [make(c) for c in choices if V(make(c).encode())]
    rej = [make(c) for c in choices if not V(make(c).encode())]
    return acc[0], rej[0]


def _luhn_family(name, rules, n, shape):
    body = _digits(random.Random(59 + n), n)
    acc, rej_last = _pick("luhn", lambda d: shape(body[:-1] + d), DIGITS)
    _, rej_first = _pick("luhn", lambda d: shape(d + acc.replace("-", "").replace(" ", "")[1:]), DIGITS)
    return (name, rules, "luhn", acc, {"last": rej_last, "first": rej_first})


def _iban_family(name, length, spaced):
    bban = iban_bbans(length)[0][1]
    shape = iban_spaced if spaced else (lambda v: v)
    acc, _ = _pick("iban", lambda chk: shape("DE" + chk + bban), IBAN_CHECKS[2:99])
    plain = acc.replace(" ", "")
    last = "0" if plain[-1] != "0" else "1"
    return (name, "short", "iban", acc, {"last": shape(plain[:-1] + last), "first": shape("E" + plain[1:])})


def alignment_families():
    """(name, rule file, validator, accepted value, {which byte differs: rejected sibling}).  A sibling differs
    from the accepted value in its last byte only, its first byte only, or (swift: the only bytes it reads) in
    byte 4 or 5.  nanp and ein read no value from the last digit: there a lost tail shows as a digit count
    short of ten or nine, which rejects the accepted value itself."""
    fam = [
        ("swift8", "short", "swift", "BANKDEFF", {"b4": "BANKQEFF", "b5": "BANKDQFF"}),
        ("swift11", "short", "swift", "BANKDEFFXXX", {"b4": "BANKQEFFXXX", "b5": "BANKDQFFXXX"}),
        ("ssn", "short", "ssn", "123-45-0001", {"last": "123-45-0000", "first": "923-45-0001"}),
        ("ein", "short", "ein", "10-1234567", {"first": "00-1234567"}),
        ("nanp_bare", "short", "nanp", "2125550187", {"first": "1125550187"}),
        ("nanp_dash", "short", "nanp", "212-555-0187", {"first": "112-555-0187"}),
        ("nanp_paren", "short", "nanp", "(212) 555-0187", {}),
        ("ipv4_7", "short", "ipv4", "1.1.1.1", {}),
        ("ipv4_12", "short", "ipv4", "10.20.30.255", {"last": "10.20.30.256"}),
        ("ipv4_12f", "short", "ipv4", "255.20.30.40", {"first": "355.20.30.40"}),
        ("ipv4_15", "short", "ipv4", "255.255.255.255", {"last": "255.255.255.256", "first": "355.255.255.255"}),
    ]
    for fname, n, shape in LUHN_FORMS:
        if fname in ("bare13", "bare16", "bare17", "bare19", "4444space", "imei2661"):
            fam.append(_luhn_family("luhn_" + fname, "short", n, shape))
    for length in (15, 16, 17, 22, 31, 32, 33, 34):
        fam.append(_iban_family("iban%d" % length, length, False))
    for length in (15, 26, 27, 30, 34):          # 18, 32, 33, 37 and 42 bytes
        fam.append(_iban_family("iban%d_spaced" % length, length, True))
    for n in (2, 3, 16, 17, 31, 32, 33, 34, 47, 48, 60):
        fam.append(_luhn_family("luhn_long_bare%d" % n, "long", n, lambda d: d))
    for n in (9, 16, 17, 24, 25, 60):            # 17, 31, 33, 47, 49 and 119 bytes
        fam.append(_luhn_family("luhn_long_sep%d" % n, "long", n, _alternate))
    for w, gaps in _widths(10):
        fam.append(("nanp_long_" + w, "long", "nanp", _spread("2125550187", "/", gaps),
                    {"first": _spread("1125550187", "/", gaps)}))
    for w, gaps in _widths(9):
        fam.append(("ssn_long_" + w, "long", "ssn", _spread("123450001", ":", gaps),
                    {"last": _spread("123450000", ":", gaps), "first": _spread("923450001", ":", gaps)}))
        fam.append(("ein_long_" + w, "long", "ein", _spread("101234567", ",", gaps),
                    {"first": _spread("001234567", ",", gaps)}))
    fam.append(("ipv4_long_15", "long", "ipv4", "255.255.255.255",
                {"last": "255.255.255.256", "first": "355.255.255.255"}))
    return fam


FILL = b"lorem ipsum dolor sit amet consectetur adipiscing elit sed do eiusmod tempor incididunt ut labore et "


def place(value: bytes, off: int, last: bool = False) -> bytes:
    """a row of a multiple of 16 bytes with the value at byte off (0 .. 15): at the row's start, or after filler
    and a space; last=True ends the row with the value instead"""
    head = b"" if off == 0 else FILL[:off - 1] + b" "
    if last:
        return head + value
    size = (len(head) + len(value) + 1 + 15) // 16 * 16
    return head + value + b" " + FILL[:size - len(head) - len(value) - 1]
