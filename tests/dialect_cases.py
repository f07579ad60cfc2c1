"""Inputs that pin the regex dialect and the hotword windows a user's dlp_config reaches the kernels with
(compiler.relax_items / build_mealy_dfa, build_first_dfa / add_first_drop / minimize, build_set_dfa;
csrc/pii_device.h first_begin / first_finish, hot_span / hot_span_pre / hot_run / hot_run_joined,
hot_rule_apply) to Python's re, through the oracle.

Plain Python: no engine, no compiler, no synth.py, no rulegen.py.  Everything is deterministic (random.Random
with fixed seeds).  test_dialect_cases.py (no GPU) checks that the lists reach what they claim to, on the oracle
alone; test_gpu_dialect.py runs them on the device.

PATTERNS   detector regexes, each with the fragments its rows are made of (matches and near-misses) and the
           literal `core` a near-miss still holds.  A pattern's own letters occur in no other pattern of its
           rule file, so within a file no two patterns can match overlapping bytes and none starves another.
HOTWORDS   hotword regex forms (used by HOT_FILE and by the lifted types)
rule_files()  name -> (dlp_config, builtin): the shipped dlp_config plus custom types and rule sets
HOT_FILE   the hotword geometry: every window size around hot_span's 4 / 16-byte steps and hot_span_pre's 64,
           fixed and relative adjustments clamped at both ends, rule order, three min_likelihood copies
first_window_rows / hot_rows / lane_rows   row builders for the runners' boundaries
"""
import json
import os
import random
import re

import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
RULES_DIR = os.path.join(os.path.dirname(HERE), "context-based-pii_amd", "rules")

LIKS = ("POSSIBLE", "LIKELY", "VERY_LIKELY")


def P(name, pattern, core, frags, **kw):
    return dict(name=name, pattern=pattern, core=core, frags=[f.encode("latin-1") for f in frags], **kw)


# file -> patterns (at most 6).  `core`: a bytes regex of the pattern's literal core; a row where it is found
# and the oracle reports no finding of the type is a near-miss.
FILES = {
    # greedy, lazy and bounded repeats of a class
    "class_repeats": [
        P("REP_EXACT", r"a\d{3}a", r"a\d", ["a123a", "a12a", "a1234a", "a123", "a999a", "aa000a"]),
        P("REP_RANGE", r"b\d{2,4}b", r"b\d", ["b12b", "b1234b", "b12345b", "b1b", "b123", "b123b"]),
        P("REP_OPEN", r"c\d{2,}c", r"c\d", ["c12c", "c1c", "c1234567c", "c12", "c123c"]),
        P("REP_RANGE_LAZY", r"d\d{1,3}?", r"d", ["d123", "d1", "d", "dd12", "d-1"]),
        P("REP_STAR_LAZY", r"e\d*?5", r"e\d*", ["e12535", "e5", "e1234", "e55", "e-5", "e05"]),
        # UNLIKELY: lifted over min_likelihood by the file's hotword rule (LIFTED)
        P("REP_PLUS_LAZY", r"f\d+?\d??g", r"f\d", ["f1g", "f12g", "f123g", "f1", "KEY f12g", "KEY f1g", "KEY f7",
                                                      "KEY  f34g"], likelihood="UNLIKELY"),
    ],
    # repeats of groups, alternations where first-wins differs from longest
    "group_repeats": [
        P("GRP_EXACT", r"(?:gh){2}i", r"gh", ["ghghi", "ghi", "ghghghi", "ghgh", "ghghii"]),
        P("GRP_RANGE", r"(?:jk){1,3}l", r"jk", ["jkl", "jkjkjkl", "jkjkjkjkl", "jk", "jkjl", "jkjkl"]),
        P("ALT_NESTED_LAZY", r"(?:m(?:n|NO)){2,}?P", r"m(?:n|NO)", ["mnmnP", "mnP", "mNOmnP", "mnmNOmnP", "mNmnP",
                                                                     "mnmn", "mNOmNOP"]),
        P("ALT_FIRST", r"p|pq|pqr", r"q", ["pqr", "pq", "p", "qr", "q", "rq"]),
        P("ALT_OPT", r"(?:st|s)(?:tu|u)?z", r"s", ["stz", "stuz", "suz", "sttuz", "stu", "sz", "stuuz", "ss"]),
        P("ALT_EMPTY", r"v(?:w|)x", r"v", ["vwx", "vx", "vwwx", "vw", "v", "vxx"]),
    ],
    # \b and \B at either end and in the middle
    "boundaries": [
        P("WB_BOTH", r"\bfoo\b", r"foo", ["foo", "foo1", "1foo", "foo_", "foo.", "-foo", "fooo"]),
        P("NB_START", r"\Bx+", r"x", ["1xx", ".x", "x", "_x", "9x.", "x-"]),
        P("WB_MID", r"s[-.]?\bs", r"s", ["s-s", "s.s", "ss", "s", "s--s", "s.s.s"]),
        P("NB_MID", r"t[-.]?\Bt", r"t", ["tt", "t-t", "t", "t.t", "ttt", "t-tt"]),
        P("WB_END", r"u\d+\b", r"u\d", ["u12", "u12a", "u1.", "u", "u12_", "u7-"]),
        P("NB_END", r"v\d\B", r"v\d", ["v1a", "v1", "v12", "v1.", "v3_", "v"]),
    ],
    # text edges, '.' with and without DOTALL, negated classes (these consume "\n" or test an edge)
    "anchors_dot": [
        P("AT_BEGIN", r"\AQ\d", r"Q\d", ["Q1", "Q2", "Q", "Q9"]),
        P("AT_END", r"z\d\Z", r"z\d", ["z1", "z2", "z", "z9"]),
        P("DOTALL", r"(?s)h.h", r"h", ["h\nh", "hah", "hh", "h-h", "h", "h\n"]),
        P("DOT", r"j.j", r"j", ["j\nj", "jaj", "jj", "j-j", "j", "j\xe9j"]),
        P("NOT_NEWLINE", r"k[^\n]k", r"k", ["k\nk", "kak", "kk", "k k", "k", "k\xffk"]),
        P("NOT_NONWORD_DIGIT", r"m[^\W\d]m", r"m", ["mam", "m_m", "m1m", "m-m", "mm", "mZm", "m\xe9m"]),
    ],
    # category classes, bytes of 0x80 and above, NOT_LITERAL, IGNORECASE on them
    "classes_bytes": [
        P("NOT_SPACE", r"n\S{2}n", r"n", ["nabn", "n  n", "n\xe9\xe9n", "na n", "n--n", "nan", "n\t.n"]),
        P("NOT_DIGIT", r"p\D+p", r"p", ["p--p", "p1p", "pabp", "p\np", "pp", "p1-p", "p\xc3\xa9p"]),
        P("HIGH_BYTES", r"q[\x80-\xff]+q", r"q", ["q\xc3\xa9q", "qq", "qaq", "q\x80q", "q\xffq", "q\x7fq",
                                                   "q\xc3\xa9"]),
        P("NOT_LITERAL", r"r[^s]r", r"r", ["rar", "rsr", "r\nr", "rr", "rSr", "r\xe9r"]),
        P("NOT_LITERAL_NOCASE", r"(?i)t[^u]t", r"[tT]", ["tat", "tut", "tUt", "TaT", "TUT", "t-T", "tt"]),
        P("HIGH_BYTE_NOCASE", r"(?i)v\xe9w", r"[vV]", ["v\xe9w", "V\xe9W", "v\xc9w", "vew", "V\xe9", "v\xe9W"]),
    ],
    # IGNORECASE global, scoped and over a range that spans the case gap; leading optional / starred group
    "case_optional": [
        P("NOCASE", r"(?i)abc\d", r"(?i)abc", ["abc1", "ABC2", "aBc3", "abcx", "ABC", "abC9"]),
        P("NOCASE_SCOPED", r"d(?i:ef)g", r"(?i)def", ["defg", "dEFg", "Defg", "defG", "dEfg", "DEFG"]),
        P("NOCASE_RANGE", r"(?i)h[X-c]h", r"[hH]", ["hxh", "hAh", "h[h", "hdh", "hWh", "HbH", "h`h", "hwh", "hCH"]),
        P("TRAIL_EXACT", r"\b\d{3,4}\b", r"\d{3}", ["123", "1234", "12345", "12", "i123", "123i", "12 345", "9876"]),
        P("LEAD_OPTIONAL", r"(?:kl)?m\d", r"m", ["klm1", "m2", "km3", "klm", "lm4", "klklm5", "m", "klmk", "mm"]),
        P("LEAD_STARRED", r"(?:no)*p\d", r"p", ["nonop1", "p1", "nop", "nop2", "onop3", "p", "nnop4"]),
    ],
    # eligible for first_drop_sets: head X+ and head X*, with and without a trailing greedy repeat; and two of
    # test_first_drop.py's ineligible neighbours
    "first_drop": [
        P("DROP_PLUS", r"a+b", r"a", ["ab", "aab", "a", "aaab", "ba", "abab", "aaa"]),
        P("DROP_STAR", r"[c-e]*f", r"[c-e]", ["cdf", "f", "cde", "ecf", "ff", "dfcf", "c"]),
        P("DROP_PLUS_TRAIL", r"g+h+", r"g", ["gh", "gghh", "g", "ggh", "hg", "ghgh", "ggg"]),
        P("DROP_STAR_TRAIL", r"[i-k]*l[m-o]+", r"l", ["ijlmn", "lm", "l", "klo", "ijl", "lmlm", "jkllo"]),
        P("NODROP_ASSERT", r"\b[pq]+@r", r"[pq]+@", ["pq@r", "p@r", "pq@", "1pq@r", "q@rr", "pp@q", "_p@r"]),
        P("NODROP_ALT", r"(?:s|t+)u", r"[st]", ["su", "ttu", "s", "tt", "stu", "ssu", "tsu"]),
    ],
    # the other ineligible neighbours, a dictionary, and a pattern of non-word bytes alone
    "first_drop_neighbours": [
        P("NODROP_BOUNDED", r"v{1,5}w", r"v", ["vw", "vvvvvw", "vvvvvvvw", "v", "vvv", "vwvw"]),
        P("NODROP_LAZY", r"x+?y", r"x", ["xy", "xxy", "x", "xxx", "yx", "xyxy"]),
        P("NODROP_BRANCH", r"z+A|B+C", r"z|B", ["zA", "zzA", "BC", "BBC", "z", "B", "zB", "zAC", "BzA"]),
        # words that are prefixes of each other and a phrase with a space
        P("DICT", None, r"(?i)mo|li", ["mo", "mona", "mona lisa", "lisa", "li", "monalisa", "MONA LISA", "Mo",
                                        "mon", "lis", "limo", "mona  lisa"],
          words=["mo", "mona", "mona lisa", "lisa", "li"]),
        # eligible, and the only one whose head class meets its last bytes: after "E#F" the start at "1#G" follows
        # a byte of the head class and is kept by the rule's second clause alone
        P("DROP_SECOND_CLAUSE", r"[E-G0-2]+#[E-G]+", r"#", ["E#F", "E#F1#G", "EF0#GE", "1#0", "2#1", "E#F0#G2#E", "0#2",
                                                             "F#G2#E"]),
        P("NONWORD_PAIR", r"\W\W\B", r"\W\W", ["--", "-+", "--1", "+-+", "==", "-"]),
    ],
    # cannot be kept apart from anything: a file of its own
    "lazy_any": [
        P("LAZY_ANY", r".+?;", r";", ["ab;", ";", "a;;", "\n;", "xyz", "a\nb;", ";", "q w;", ";\n", "\n"], n=400),
    ],
}
# the types below POSSIBLE, and the hotword rule of their file that lifts them
LIFTED = {"REP_PLUS_LAZY": dict(file="class_repeats", hotword=r"\bKEY\b", window_before=6, relative=2)}

for _f, _ps in FILES.items():
    for _p in _ps:
        _p["file"] = _f
PATTERNS = {p["name"]: p for ps in FILES.values() for p in ps}

# the four patterns compile_rules used to reject: the SCAN prefix reaches an optional or starred group of
# several items before any required character
FORMERLY_REJECTED = [r"(?:\+1[ -])?\d{3}-\d{4}", r"(?:ab)?c\d", r"(?:ab)*c\d", r"a{0,1}(?:ab){0,1}b\d"]
# the same shape with the optional group last in a plain group: its rest is what follows that group
REJECTED_IN_GROUP = [r"((?:xy)?)z\d", r"(?:w(?:xy)*)?(z[0-9])"]
# ... and last in a group that sets a flag, which the relaxation does not open: still refused
STILL_REFUSED = [r"(?i:(?:ab)?)c\d"]
REJECTED_FRAGS = [b"+1 555-1234", b"555-1234", b"+1-555-12", b"abc1", b"c2", b"ababc3", b"abab", b"aabb4", b"abb5",
                  b"b6", b"ab7", b"a", b" ", b"+1", b"ac8", b"xyz1", b"z2", b"xy", b"wxyz3",
                  b"wz4", b"xz"]

# hotword regex forms: \b..\b, \A.., ..\Z, a one-byte class, bytes of 0x80 and above, a two-word phrase,
# (?:no|not)\s+a
HOTWORDS = [r"\bzq\b", r"\AZa", r"Zb\Z", r"[%]", r"\xc3\xa9", r"hw f", r"(?:no|not)\s+a"]


def _shipped():
    with open(os.path.join(RULES_DIR, "dlp_config.json")) as f:
        cfg = json.load(f)
    with open(os.path.join(RULES_DIR, "builtin_infotypes.yaml")) as f:
        builtin = yaml.safe_load(f)
    return cfg, builtin


def _custom(p, k):
    c = {"info_type": {"name": p["name"]}, "likelihood": p.get("likelihood", LIKS[k % 3])}
    if p.get("words"):
        c["dictionary"] = {"word_list": {"words": list(p["words"])}}
    else:
        c["regex"] = {"pattern": p["pattern"]}
    return c


def detector_regex(p) -> "re.Pattern":
    """the bytes regex the oracle and the compiler give the custom type"""
    if p.get("words"):
        return re.compile((r"(?i)\b(?:" + "|".join(re.escape(w) for w in p["words"]) + r")\b").encode("ascii"))
    return re.compile(p["pattern"].encode("ascii"))


def _hot_rule(pattern, wb, wa, fixed=None, relative=None):
    adj = {}
    if fixed is not None:
        adj["fixed_likelihood"] = fixed
    if relative is not None:
        adj["relative_likelihood"] = relative
    prox = {}
    if wb:
        prox["window_before"] = wb
    if wa:
        prox["window_after"] = wa
    return {"hotword_rule": {"hotword_regex": {"pattern": pattern}, "proximity": prox, "likelihood_adjustment": adj}}


# ----------------------------------------------------------------------------------------- HOT_FILE
# HOT: a fixed-length detector of 16 bytes, POSSIBLE, with fifteen rules, one per window size, each with a
# hotword of its own so that a row's one hotword says which rule decides.  (text of the hotword as the rows
# write it, regex, window, fixed, relative)
HOT_DET = r"<[g-p]{14}>"
HOT_MATCH = b"<ghijklmnopghij>"
HOT_RULES = [
    (b"%", r"[%]", 1, None, 1),
    (b"\xc3\xa9", r"\xc3\xa9", 2, None, 4),
    (b"zq", r"\bzq\b", 3, "VERY_LIKELY", None),
    (b"Za", r"\AZa", 4, None, -1),
    (b"Zb", r"Zb\Z", 5, None, -4),
    (b"hwc", r"\bhwc\b", 15, "VERY_UNLIKELY", None),
    (b"hwd", r"hwd\Z", 16, None, 1),
    (b"hwe", r"\Ahwe", 17, "VERY_LIKELY", None),
    (b"hw f", r"hw f", 31, None, 4),
    (b"not\t a", r"(?:no|not)\s+a", 32, None, -1),
    (b"hwg", r"\bhwg\b", 33, None, 1),
    (b"hwh", r"\bhwh\b", 63, "VERY_LIKELY", None),
    (b"hwi", r"hwi\Z", 64, None, -4),
    (b"hwj", r"\Ahwj", 65, "VERY_UNLIKELY", None),
    (b"hwk", r"\bhwk\b", 300, None, 4),
]
HOT_SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 300]
# ORD: three rules on one type whose result depends on their order -- relative, then fixed, then relative.  The
# fixed one states a relative adjustment too, which a fixed likelihood overrides.
ORD_DET = r"\[[g-p]{14}\]"
ORD_MATCH = b"[ghijklmnopghij]"
ORD_RULES = [(b"oa", r"\boa\b", 40, None, -1), (b"ob", r"\bob\b", 40, "LIKELY", -2), (b"oc", r"\boc\b", 40, None, -1)]
# FW: the detector of first_window_rows (match lengths 1 .. 40)
FW_DET = r"Q[a-z]*\d?"
HOT_FILE = "hot"
# the files none of whose detectors consumes "\n" or tests a text edge (compiler: window_ok): their windows can be
# re-scanned incrementally
WINDOW_FILES = ["hot", "class_repeats", "group_repeats", "boundaries", "case_optional", "first_drop", "lazy_any"]
HOT_COPIES = {"hot": None, "hot_likely": "LIKELY", "hot_very_unlikely": "VERY_UNLIKELY"}
FILL = b".,:-+/=*()"          # non-word filler: no hotword, no detector of the hot file, never two alike in a row


def fill(n: int, phase: int = 0) -> bytes:
    return bytes(FILL[(phase + i) % len(FILL)] for i in range(n))


def _hot_config(min_likelihood):
    cfg, builtin = _shipped()
    insp = cfg["inspect_config"]
    # build-defined detectors listed in info_types, not custom types: a context record naming one changes its
    # rules (main.py:637-686) -- HOT's first rule becomes fixed VERY_LIKELY, FW gets the ".+" 100 / 100 rule
    for name, pat, lik in (("HOT", HOT_DET, "POSSIBLE"), ("ORD", ORD_DET, "LIKELY"), ("FW", FW_DET, "LIKELY")):
        builtin["detectors"][name] = [{"pattern": pat, "likelihood": lik}]
        insp["info_types"].append({"name": name})
    # HOT's rule set first: its fifteen rules are the engine's hotword rules 0 .. 14, the ones the window path
    # keeps resident bits for (16 of them), so the windows of 64, 65 and 300 bytes reach k_win_halo's
    # hot_span_pre too; ORD's and the shipped rules after them take the window path's other branch
    insp["rule_set"] = [
        {"info_types": [{"name": "HOT"}], "rules": [_hot_rule(rx, w, w, fx, rel) for _, rx, w, fx, rel in HOT_RULES]},
        {"info_types": [{"name": "ORD"}], "rules": [_hot_rule(rx, w, w, fx, rel) for _, rx, w, fx, rel in ORD_RULES]},
    ] + list(insp.get("rule_set") or [])
    if min_likelihood is not None:
        insp["min_likelihood"] = min_likelihood
    return cfg, builtin


def rule_files():
    """name -> (dlp_config, builtin): the shipped rules plus the file's custom types and rule sets (written to
    disk by write_rules, loaded from there like a user's)"""
    out = {}
    for name, ps in FILES.items():
        assert len(ps) <= 6
        cfg, builtin = _shipped()
        insp = cfg["inspect_config"]
        insp.setdefault("custom_info_types", []).extend(_custom(p, k) for k, p in enumerate(ps))
        for t, lift in LIFTED.items():
            if lift["file"] == name:
                insp.setdefault("rule_set", []).append({"info_types": [{"name": t}], "rules": [
                    _hot_rule(lift["hotword"], lift["window_before"], 0, relative=lift["relative"])]})
        out[name] = (cfg, builtin)
    for name, ml in HOT_COPIES.items():
        out[name] = _hot_config(ml)
    assert len(out) <= 12
    return out


def own_types(name):
    if name in HOT_COPIES:
        return ["HOT", "ORD", "FW"]
    return [p["name"] for p in FILES[name]]


def write_rules(tmp_dir, name, pair):
    """(dlp_config path, builtin path) of one rule file pair written into tmp_dir (validator_cases.write_rules'
    form)"""
    cfg, builtin = pair
    cfg_path = os.path.join(str(tmp_dir), name + "_dlp_config.json")
    builtin_path = os.path.join(str(tmp_dir), name + "_builtin.yaml")
    with open(cfg_path, "w") as f:
        json.dump(cfg, f)
    with open(builtin_path, "w") as f:
        yaml.safe_dump(builtin, f)
    return cfg_path, builtin_path


# ------------------------------------------------------------------------------------- dialect rows
SEPS = [b" ", b" ", b"", b". ", b" , "]
# NONWORD_PAIR would match the longer separators; LAZY_ANY takes every byte but "\n" before a ';'
FILE_SEPS = {"first_drop_neighbours": [b" ", b""], "lazy_any": [b"\n", b"\n", b"\n", b" "]}
# the shipped detectors and hotwords beside the custom types: appended to every file's rows
SHIPPED_ROWS = [b"my ssn is 536-22-8726 ok", b"credit card 4111 1111 1111 1111 cvv 123", b"the ip address is 10.20.30.40",
                b"phone number 212-555-0187, mail a.b@c.de", b"card number: 4111-1111-1111-1111", b"passport 123456789",
                b"no hotword 536-22-8726 and 10.20.30.40 or 123"]


def pattern_rows(p):
    """rows of the pattern's own fragments alone"""
    n = p.get("n", 160)
    rnd = random.Random(sum(p["name"].encode()) * 7919)
    rows = [bytes(f) for f in p["frags"]]
    while len(rows) < n:
        k = rnd.randrange(1, 6)
        row = b""
        for i in range(k):
            row += rnd.choice(p["frags"])
            if i + 1 < k:
                row += rnd.choice(FILE_SEPS.get(p["file"], SEPS))
        rows.append(row)
    return rows


def file_rows(name, mixed=200):
    """(label, row): every pattern's own rows, then rows that mix the file's patterns (single spaces between
    fragments), a few of them long enough for first_finish and the scan lanes' cut"""
    ps = FILES[name]
    out = []
    for p in ps:
        out += [("%s/%d" % (p["name"], i), r) for i, r in enumerate(pattern_rows(p))]
    if len(ps) > 1:
        rnd = random.Random(len(name) * 104729)
        for i in range(mixed):
            k = rnd.randrange(2, 9) if i % 10 else rnd.randrange(30, 60)
            row = b" ".join(rnd.choice(rnd.choice(ps)["frags"]) for _ in range(k))
            out.append(("mixed/%d" % i, row))
    out += [("shipped/%d" % i, r) for i, r in enumerate(SHIPPED_ROWS)]
    return out


# --------------------------------------------------------------------------- first_begin / first_finish
FW_LENGTHS = list(range(1, 41))
FW_STARTS = list(range(18))
FW_TAILS = [0, 1, 2, 15, 16, 17]


def fw_match(n: int) -> bytes:
    if n == 1:
        return b"Q"
    return b"Q" + bytes(97 + (i * 7) % 26 for i in range(n - 2)) + b"7"


def first_window_rows(pattern=FW_DET):
    """(label, row, start, match length) for a detector `pattern` that matches fw_match(n) whole, and all but
    its last byte when a '-' stands there (FW's Q[a-z]*\\d?: every state accepts, and the run ends where the
    digit or the '-' stands, which over the lengths and starts below is every position of the window).
    The match of every length 1 .. 40 at every start 0 .. 17, the row ending 0, 1, 2, 15, 16 or 17 bytes after
    it; each with a sibling that differs in the last matching byte only (its match is one byte shorter, or
    gone).  first_begin consumes the byte before the start and 15 more: lengths up to 15 / 16 end in its window
    (the end-of-text test when the row ends there), longer ones hand a saved state at start + 15 to
    first_finish, whose chunks are of every length 1 .. 16."""
    rx = re.compile(pattern.encode("ascii"))
    for n in FW_LENGTHS:
        m, sib = fw_match(n), rx.match(fw_match(n)[:-1] + b"-")
        assert rx.fullmatch(m) and (sib.end() if sib else 0) == n - 1, (pattern, n)
    out = []
    for n in FW_LENGTHS:
        m = fw_match(n)
        for s in FW_STARTS:
            for t in FW_TAILS:
                pre, post = fill(s, n), fill(t, s + 1)
                out.append(("fw/%d/%d/%d" % (n, s, t), pre + m + post, s, n))
                out.append(("fw/%d/%d/%d/sib" % (n, s, t), pre + m[:-1] + b"-" + post, s, n - 1))
    return out


# ------------------------------------------------------------------------------------- hotword rows
def _distances(w, ln):
    return sorted({d for d in (0, 1, w - ln, w - ln + 1, w, w + 1) if d >= 0})


def hot_rows():
    """(label, row, rule index, side).  For every rule of HOT (window w, hotword of ln bytes) the hotword ends d
    bytes before the match start, d in {0, 1, w - ln, w - ln + 1, w, w + 1} -- and begins d bytes after the match
    end -- at each start offset 0 .. 15 of the hotword (a prefix of non-word filler); offset 0 with the hotword
    first (or last) in the row is the window clipped by the row, where \\A, \\Z and \\b are decided by the clip.
    Then ORD's rows: every subset of its three hotwords before the match."""
    out = []
    for k, (text, _rx, w, _fx, _rel) in enumerate(HOT_RULES):
        ln = len(text)
        for d in _distances(w, ln):
            for off in range(16):
                out.append(("hot/%d/before/d%d/o%d" % (k, d, off),
                            fill(off, k) + text + fill(d, off + 1) + HOT_MATCH + fill(off % 3, 2), k, "before"))
                out.append(("hot/%d/after/d%d/o%d" % (k, d, off),
                            fill(off, k) + HOT_MATCH + fill(d, off + 1) + text + fill(off % 4, 5), k, "after"))
            # the clip with word bytes beyond it: the hotword's \b / \A / \Z inside a longer word or row
            out.append(("hot/%d/before/d%d/word" % (k, d), b"x" + text + fill(d, 1) + HOT_MATCH, k, "before"))
            out.append(("hot/%d/after/d%d/word" % (k, d), HOT_MATCH + fill(d, 1) + text + b"x", k, "after"))
    for mask in range(8):
        for gap in (1, 7, 30):
            for off in (0, 5, 11):
                words = b" ".join(t for i, (t, *_r) in enumerate(ORD_RULES) if (mask >> i) & 1)
                out.append(("ord/%d/g%d/o%d" % (mask, gap, off),
                            fill(off, mask) + words + fill(gap, 3) + ORD_MATCH + fill(2, 1), -1, "before"))
                out.append(("ord/%d/g%d/o%d/after" % (mask, gap, off),
                            fill(off, mask) + ORD_MATCH + fill(gap, 3) + words + fill(1, 1), -1, "after"))
    return out


def hot_rule_hit(k, row, s, e, grow=0):
    """rule k of HOT on the match [s, e) of row, by re.search on the slices (window + grow bytes)"""
    _text, rx, w, _fx, _rel = HOT_RULES[k]
    r = re.compile(rx.encode("ascii"))
    w += grow
    return bool(r.search(row[max(0, s - w):s]) or r.search(row[e:e + w]))


# ---------------------------------------------------------------------------------------- lane rows
def lane_rows():
    """(label, row): a hotword, the window between and a match of HOT placed so that byte `cut` falls inside the
    hotword, inside the gap and inside the match -- cut = 1024 in rows of 1000 .. 2200 bytes (the scan lanes of
    long rows), 128 in rows of 120 .. 140 and 256 in rows of 250 .. 262 bytes (rows cut at a lane)."""
    out = []
    picks = [k for k, r in enumerate(HOT_RULES) if r[2] in (17, 33, 63, 64, 65, 300)]
    for cut, sizes in ((1024, (1000, 1023, 1024, 1025, 1040, 1500, 2200)), (128, (120, 127, 128, 129, 140)),
                       (256, (250, 255, 256, 257, 262))):
        for k in picks:
            text, _rx, w, _fx, _rel = HOT_RULES[k]
            for d in (0, w - len(text), w - len(text) + 1):
                unit = text + fill(d, 1) + HOT_MATCH
                if len(unit) > min(sizes) - 4 and cut != 1024:
                    continue
                for at in sorted({1, len(text), len(text) + d // 2, len(text) + d, len(text) + d + 1,
                                  len(text) + d + 8, len(unit) - 1}):
                    if at > cut or at >= len(unit):
                        continue
                    rev = HOT_MATCH + fill(d, 1) + text
                    for size in sizes:
                        # byte `cut` of the row is byte `at` of the unit; a row too short for that ends with it
                        head = fill(min(cut - at, size - len(unit)), k)
                        for side, u in (("before", unit), ("after", rev)):
                            out.append(("lane/%d/%d/d%d/at%d/%d/%s" % (cut, k, d, at, size, side),
                                        head + u + fill(size - len(head) - len(u), 4)))
    return out
