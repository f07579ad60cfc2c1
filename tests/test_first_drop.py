"""Absorbed match starts (compiler.first_drop_sets / first_drop / add_first_drop).

A pattern X{lo,}.rest with a greedy unbounded class repeat as its head matches at s - 1 whenever it
matches at s and text[s-1] is in X, with the same end, so finditer skips s -- unless an earlier match
ends exactly at s.  The compiler's rule drops s before its FIRST run iff
    text[s-1] in X and not (text[s-1] in Z and text[s] not in G).
Checked here against re.finditer: the matched starts that survive the rule, run through k_select's
skip (a start inside the pattern's previous match is ignored), must be exactly finditer's matches.
The emitted PRE row / extra start states of the FIRST automaton are checked against the same rule.
"""
import random
import re

import numpy as np
import pytest

from conftest import pkg

EMAIL_ALPHABET = b"ab1.@- _%Z"
COUNTEREXAMPLE = b"@-@11.aa-.@1-.bZ1.%._1"
FRAGMENTS = [b"a", b"b1", b".com", b"x@y.org", b"@", b".", b"-", b" ", b"Z9", b"a.b@c.de", b"%", b"_", b"1"]

# (pattern, alphabet of <= 10 characters, fragments)
HANDMADE = [
    (r"a+b", b"ab c", [b"a", b"ab", b"b", b" ", b"aab", b"c"]),
    (r"[a-z]+@[a-z]+\.[a-z]{2,}", b"abz@. 1", FRAGMENTS),
    (r"[a-z]*\d", b"ab19 -", [b"a", b"1", b"ab", b" ", b"b9", b"-", b"zz"]),
    (r"[a-c]+\.\d", b"abc.12 ", [b"a", b".1", b"bc", b" ", b"c.2", b".", b"2"]),          # Z & X empty
    (r"[a-z0-9]+@[a-z]+", b"ab12@ .", [b"a", b"1", b"@b", b"a@b", b" ", b"2@a1", b".", b"b2"]),
]
NOT_ELIGIBLE = [r"\b\w+@x", r"(?:a|b+)c", r"a{1,5}b", r"a+?b", r"a+b|c+d"]


def _random_strings(r, alphabet, n, lo=1, hi=28):
    return [bytes(r.choice(alphabet) for _ in range(r.randrange(lo, hi))) for _ in range(n)]


def _fragment_strings(r, fragments, n):
    return [b"".join(r.choice(fragments) for _ in range(r.randrange(1, 12))) for _ in range(n)]


def _matched_starts(rx, text):
    out = []
    for s in range(len(text)):
        m = rx.match(text, s)
        if m:
            out.append((s, m.end()))
    return out


def _select(starts):
    """k_select's finditer skip over one pattern's matched (start, end) list"""
    out, prev_end = [], -1
    for s, e in starts:
        if s < prev_end:
            continue
        prev_end = e
        out.append((s, e))
    return out


def _check_pattern(comp, pattern, texts):
    sets = comp.first_drop_sets(pattern)
    assert sets is not None, pattern
    x, z, g = sets
    rx = re.compile(pattern.encode())
    n_matched = n_dropped = n_second = 0
    for t in texts:
        starts = _matched_starts(rx, t)
        want = [m.span() for m in rx.finditer(t)]
        assert _select(starts) == want, (pattern, t)               # the skip logic itself
        kept = [(s, e) for s, e in starts if not comp.drop_start(sets, t, s)]
        assert _select(kept) == want, (pattern, t, starts, kept)
        n_matched += len(starts)
        n_dropped += len(starts) - len(kept)
        n_second += sum(1 for s, _ in kept if s > 0 and (x >> t[s - 1]) & 1)
    assert n_matched >= 1000, (pattern, n_matched)
    assert n_dropped > 0, pattern
    # a start after a byte of X is kept only by the second clause; that needs text[s-1] in X & Z and
    # text[s] (a byte of X, the start matched) outside G -- impossible when X & Z or X - G is empty
    if (x & z) and (x & ~g):
        assert n_second > 0, pattern
    else:
        assert n_second == 0, pattern
    return n_matched, n_dropped, n_second


@pytest.mark.parametrize("pattern,alphabet,fragments", HANDMADE, ids=[h[0] for h in HANDMADE])
def test_rule_vs_finditer_handmade(pattern, alphabet, fragments):
    comp = pkg("compiler")
    r = random.Random(11)
    texts = _random_strings(r, alphabet, 3000) + _fragment_strings(r, fragments, 1500)
    _check_pattern(comp, pattern, texts)


def test_rule_vs_finditer_shipped(compiled):
    comp = pkg("compiler")
    eligible = [p for p in compiled.rules.patterns if comp.first_drop_sets(p.pattern) is not None]
    assert "EMAIL_ADDRESS" in [p.type_name for p in eligible]
    pre = compiled.sections["det.first_pre"]
    assert [int(v) >= 0 for v in pre] == [comp.first_drop_sets(p.pattern) is not None for p in compiled.rules.patterns]
    r = random.Random(12)
    texts = _random_strings(r, EMAIL_ALPHABET, 6000) + _fragment_strings(r, FRAGMENTS, 3000) + [COUNTEREXAMPLE]
    for p in eligible:
        _check_pattern(comp, p.pattern, texts)


def test_naive_rule_fails_on_the_counterexample(compiled):
    """dropping every start after a byte of X loses the match that resumes where the previous ended"""
    comp = pkg("compiler")
    pat = next(p.pattern for p in compiled.rules.patterns if p.type_name == "EMAIL_ADDRESS")
    sets = comp.first_drop_sets(pat)
    rx = re.compile(pat.encode())
    t = COUNTEREXAMPLE
    want = [m.span() for m in rx.finditer(t)]
    assert want == [(1, 8), (8, 16)]
    starts = _matched_starts(rx, t)
    naive = [(s, e) for s, e in starts if not (s > 0 and (sets[0] >> t[s - 1]) & 1)]
    assert _select(naive) != want
    assert _select([(s, e) for s, e in starts if not comp.drop_start(sets, t, s)]) == want


@pytest.mark.parametrize("pattern", NOT_ELIGIBLE)
def test_not_eligible(pattern):
    assert pkg("compiler").first_drop_sets(pattern) is None


def _table_run(d, pre, text, s):
    """first_begin / first_finish over the DFA's tables, the start state taken from the PRE row"""
    ncls = d.n_classes
    if s == 0:
        st = d.start[0]
    else:
        st = int(d.trans[pre, d.cmap[text[s - 1]]])
        if d.flags[st] & 2:
            return -1
    last = -1
    for j in range(s, len(text)):
        st = int(d.trans[st, d.cmap[text[j]]])
        if d.flags[st] & 1:
            last = j
        if d.flags[st] & 2:
            return last
    if d.flags[int(d.trans[st, ncls])] & 1:
        last = len(text)
    return last


def test_pre_row_is_the_rule(compiled):
    """the PRE row and its extra start states give -1 for a dropped start and re's end otherwise"""
    comp = pkg("compiler")
    r = random.Random(13)
    cases = [(p.pattern, compiled.first[p.pid], int(compiled.sections["det.first_pre"][p.pid]))
             for p in compiled.rules.patterns if compiled.sections["det.first_pre"][p.pid] >= 0]
    for pattern, _, _ in HANDMADE:
        nfa = comp.NFA()
        d = comp.build_first_dfa(nfa, comp.add_pattern(nfa, pattern, 0, reverse=False))
        n0 = d.n_states
        d2, pre = comp.add_first_drop(d, comp.first_drop_sets(pattern))
        assert np.array_equal(d2.trans[:n0], d.trans) and np.array_equal(d2.flags[:n0], d.flags)
        cases.append((pattern, d2, pre))
    assert len(cases) > len(HANDMADE)
    alphabets = {h[0]: h[1] for h in HANDMADE}
    for pattern, d, pre in cases:
        sets = comp.first_drop_sets(pattern)
        rx = re.compile(pattern.encode())
        n_drop = n_match = 0
        for t in _random_strings(r, alphabets.get(pattern, EMAIL_ALPHABET), 600) + [COUNTEREXAMPLE]:
            for s in range(len(t)):
                m = rx.match(t, s)
                dropped = comp.drop_start(sets, t, s)
                want = -1 if dropped or not m else m.end()
                assert _table_run(d, pre, t, s) == want, (pattern, t, s)
                n_drop += bool(dropped and m)
                n_match += bool(m)
        assert n_drop > 0 and n_match > n_drop, pattern


def test_blob_round_trip_keeps_the_section(compiled):
    comp = pkg("compiler")
    S = comp.blob_sections(compiled.blob)
    assert S["det.first_pre"].dtype == np.int32 and len(S["det.first_pre"]) == len(compiled.rules.patterns)
    desc = S["det.first_desc"].reshape(-1, 8)
    for p, pre in enumerate(S["det.first_pre"]):
        assert -1 <= int(pre) < int(desc[p, 7])
