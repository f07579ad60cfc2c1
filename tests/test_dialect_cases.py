"""The regex dialect and the hotword geometry on the CPU: the lists of dialect_cases reach what they claim to
(conditions on the inputs, checked under the oracle alone), and the compiled tables, run the way the kernels run
them (tests/tablesim.py), agree with Python's re and with the oracle on every row.  test_gpu_dialect.py runs the
same lists on the device.  The counts printed here (pytest -s) are recorded in profiles/dialect/README.txt."""
import re

import pytest

import dialect_cases as DC
from conftest import pkg

FILE_NAMES = list(DC.FILES)
ALL_NAMES = FILE_NAMES + list(DC.HOT_COPIES)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """rule file name -> (oracle RuleConfig, compiled rules, TableSim), loaded from files as a user's would be"""
    from oracle import pii_oracle as O
    from tablesim import TableSim
    comp = pkg("compiler")
    d = tmp_path_factory.mktemp("dialect")
    made = {}

    def get(name):
        if name not in made:
            cfg, builtin = DC.write_rules(d, name, DC.rule_files()[name])
            c = comp.compile_default(cfg, builtin)
            made[name] = (O.RuleConfig.load(cfg, builtin), c, TableSim(c))
        return made[name]
    return get


def _rows_of(name):
    if name in DC.HOT_COPIES:
        return [(label, row) for label, row, *_ in DC.hot_rows()]
    return DC.file_rows(name)


def _pid(comp, type_name):
    return next(p.pid for p in comp.rules.patterns if p.type_name == type_name)


# ------------------------------------------------------------------------------ the lists themselves
def test_the_lists_hold_what_the_issue_asks_for():
    assert len(DC.PATTERNS) >= 40 and sum(len(ps) for ps in DC.FILES.values()) == len(DC.PATTERNS)
    assert len(DC.rule_files()) <= 12 and all(len(ps) <= 6 for ps in DC.FILES.values())
    for name, p in DC.PATTERNS.items():
        low = p.get("likelihood") in ("UNLIKELY", "VERY_UNLIKELY")
        assert low == (name in DC.LIFTED), name
    sizes = {w for _, _, w, _, _ in DC.HOT_RULES}
    assert sizes == set(DC.HOT_SIZES) == {1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 300}
    adj = {(fx, rel) for _, _, _, fx, rel in DC.HOT_RULES}
    assert {("VERY_UNLIKELY", None), ("VERY_LIKELY", None), (None, -4), (None, -1), (None, 1), (None, 4)} <= adj
    assert [(fx is None) for _, _, _, fx, _ in DC.ORD_RULES] == [True, False, True]   # relative, fixed, relative
    for ln, w in ((len(t), w) for t, _, w, _, _ in DC.HOT_RULES):
        assert ln <= w
    # a hotword form of every kind is in use
    used = {rx for _, rx, *_ in DC.HOT_RULES}
    assert set(DC.HOTWORDS) <= used
    rows = DC.first_window_rows()
    assert {(s, n) for _, _, s, n in rows if n > 0} >= {(s, n) for s in range(18) for n in range(1, 41)}
    lane = [len(r) for _, r in DC.lane_rows()]
    assert min(lane) >= 120 and max(lane) <= 2200 and any(1000 <= n for n in lane)
    assert any(120 <= n <= 140 for n in lane) and any(250 <= n <= 262 for n in lane)
    assert max(len(r) for _, r, *_ in DC.hot_rows()) < 2200


def test_window_files_are_the_ones_the_compiler_allows(files):
    ok = [n for n in ALL_NAMES if int(files(n)[1].sections["meta"][13]) == 1]
    assert sorted(ok) == sorted(DC.WINDOW_FILES + ["hot_likely", "hot_very_unlikely"])
    assert {len(files(n)[1].scan_groups) for n in ALL_NAMES} == {1, 2}            # one and two SCAN groups
    # HOT's rules are the hot file's hotword rules 0 .. 14: below the sixteen the window path keeps bits for
    hot = files(DC.HOT_FILE)[1].hot_rules
    assert [(h.pattern, h.window_before) for h in hot[:15]] == [(rx, w) for _, rx, w, _, _ in DC.HOT_RULES]
    assert len(hot) > 16


@pytest.mark.parametrize("name", [n for n in FILE_NAMES if len(DC.FILES[n]) > 1])
def test_no_pattern_matches_in_the_rows_of_another_of_its_file(name):
    ps = DC.FILES[name]
    for p in ps:
        rows = DC.pattern_rows(p)
        for q in ps:
            if q is not p:
                rx = DC.detector_regex(q)
                assert not any(rx.search(r) for r in rows), (p["name"], q["name"])


# ----------------------------------------------------------------------------- reach, on the oracle
@pytest.mark.parametrize("name", FILE_NAMES)
def test_every_type_is_found_and_nearly_found(name, files):
    from oracle import pii_oracle as O
    ocfg = files(name)[0]
    rows = DC.file_rows(name)
    found = [O.find_pii(r, ocfg) for _, r in rows]
    for p in DC.FILES[name]:
        tid = ocfg.type_id[p["name"]]
        core = re.compile(p["core"].encode("latin-1"))
        n_found = sum(f.type_id == tid for fs in found for f in fs)
        n_near = sum(1 for (_, r), fs in zip(rows, found)
                     if core.search(r) and not any(f.type_id == tid for f in fs))
        print("reach %-22s %-20s findings %4d near-misses %4d" % (name, p["name"], n_found, n_near))
        assert n_found >= 30, p["name"]
        assert n_near >= 30, p["name"]
    for t, lift in DC.LIFTED.items():
        if lift["file"] == name:                      # lifted in some rows, under min_likelihood in others
            tid = ocfg.type_id[t]
            rx = DC.detector_regex(DC.PATTERNS[t])
            n_match = sum(len(rx.findall(r)) for _, r in rows)
            n_found = sum(f.type_id == tid for fs in found for f in fs)
            assert 30 <= n_found <= n_match - 30, (t, n_found, n_match)


def _hot_geometry():
    """per hot row of a HOT rule: (rule, side, offset label, d, hit by re.search on the slices)"""
    out = []
    det = re.compile(DC.HOT_DET.encode())
    for label, row, k, side in DC.hot_rows():
        if k < 0:
            continue
        m = det.search(row)
        parts = label.split("/")
        out.append((k, side, parts[4], int(parts[3][1:]), DC.hot_rule_hit(k, row, m.start(), m.end())))
    return out


def test_every_hot_rule_hits_and_misses_by_one_byte():
    geo = _hot_geometry()
    hits = {(k, side, off, d) for k, side, off, d, hit in geo if hit}
    for k in range(len(DC.HOT_RULES)):
        n_hit = sum(1 for g in geo if g[0] == k and g[4])
        # a miss whose neighbour (the hotword one byte nearer or farther, all else equal) is a hit
        n_miss = sum(1 for kk, side, off, d, hit in geo if kk == k and not hit and
                     ((k, side, off, d - 1) in hits or (k, side, off, d + 1) in hits))
        print("reach hot rule %2d w=%3d %-18s hits %3d misses by one byte %3d" % (
            k, DC.HOT_RULES[k][2], DC.HOT_RULES[k][1], n_hit, n_miss))
        assert n_hit >= 5 and n_miss >= 5, k
        for side in ("before", "after"):
            assert any(g[0] == k and g[1] == side and g[4] for g in geo), (k, side)
    # windows clipped by the row decide \A, \Z and \b: the same distance hits at offset 0 and misses at another
    for k, (_t, rx, *_r) in enumerate(DC.HOT_RULES):
        if "\\A" in rx or "\\Z" in rx:
            by = {}
            for kk, side, off, d, hit in geo:
                if kk == k:
                    by.setdefault((side, d), set()).add((off == "o0", hit))
            assert any({(True, True), (False, False)} <= v for v in by.values()), rx


def test_the_min_likelihood_copies_differ(files):
    from oracle import pii_oracle as O
    rows = [r for _, r, *_ in DC.hot_rows()]
    found = {}
    for name in DC.HOT_COPIES:
        ocfg = files(name)[0]
        assert ocfg.min_likelihood == O.lik_value(DC.HOT_COPIES[name] or "POSSIBLE")
        found[name] = {(i, f.start, f.end, f.type_id, f.likelihood) for i, r in enumerate(rows)
                       for f in O.find_pii(r, ocfg)}
    names = list(DC.HOT_COPIES)
    for a in range(3):
        for b in range(a + 1, 3):
            n = len(found[names[a]] ^ found[names[b]])
            print("reach min_likelihood %s / %s: %d findings change" % (names[a], names[b], n))
            assert n >= 20
    # every likelihood 1 .. 5 is reached by HOT, and ORD's result depends on the order of its rules
    ocfg = files("hot_very_unlikely")[0]
    tid = ocfg.type_id["HOT"]
    assert {lk for _, _, _, t, lk in found["hot_very_unlikely"] if t == tid} == {1, 2, 3, 4, 5}
    oid = ocfg.type_id["ORD"]
    assert {lk for _, _, _, t, lk in found["hot_very_unlikely"] if t == oid} == {2, 3, 4}


# ------------------------------------------------------------------------------------------ runners
def _reported(sim, text):
    """start -> pattern ids the SCAN automata of every group report there"""
    out = {}
    for pos, sd, _sk in sim.scan(text, True):
        a = sim.d_accept(text, pos, sd)
        out.setdefault(pos, set()).update(int(sim.d_ids[i]) for i in range(int(sim.d_off[a]), int(sim.d_off[a + 1])))
    return out


def _check_first_and_scan(sim, comp, rows, type_names):
    pats = [(p.pid, p.type_name, re.compile(p.pattern.encode("ascii"))) for p in comp.rules.patterns]
    own = {_pid(comp, t) for t in type_names}
    n_runs = 0
    for _, t in rows:
        rep = _reported(sim, t)
        for pid, tname, rx in pats:
            for s in range(len(t) + 1):
                m = rx.match(t, s)
                if pid in own:                                  # FIRST after minimize and add_first_drop
                    assert sim.first_run(pid, t, s) == (m.end() if m else -1), (tname, t, s)
                    n_runs += 1
                if m and m.end() > s:                           # the relaxed reverse SCAN: a superset of starts
                    assert pid in rep.get(s, ()), (tname, t, s)
    return n_runs


@pytest.mark.parametrize("name", FILE_NAMES)
def test_first_and_scan_against_re_at_every_start(name, files):
    _, comp, sim = files(name)
    assert _check_first_and_scan(sim, comp, DC.file_rows(name), DC.own_types(name)) > 2000


@pytest.mark.parametrize("rows", ["first_window", "hot", "lane"])
def test_first_and_scan_on_the_window_hotword_and_lane_rows(rows, files):
    _, comp, sim = files("hot")
    lists = {"first_window": lambda: [(label, r) for label, r, *_ in DC.first_window_rows()],
             "hot": lambda: _rows_of("hot"), "lane": DC.lane_rows}
    assert _check_first_and_scan(sim, comp, lists[rows](), DC.own_types("hot")) > 100000


def _hot_tables(sim, h):
    """the automaton of hotword rule h as plain lists: transitions, flags, byte classes, columns, start"""
    tr, fl, cm, nc, s0, _, _, ns = [int(x) for x in sim.hot_desc[h]]
    return (sim.ptrans[tr:tr + ns * nc].tolist(), sim.pflags[fl:fl + ns].tolist(), sim.pcmap[cm:cm + 256].tolist(),
            nc, s0)


def _hot_prefix_accepts(tables, seg):
    """TableSim.hot_run(h, seg[:n]) for every n in one pass"""
    T, F, M, nc, st = tables
    hit, out = False, []
    for c in seg:
        out.append(hit or bool(F[T[st * nc + nc - 1]]))
        st = T[st * nc + M[c]]
        hit = hit or bool(F[st])
    out.append(hit or bool(F[T[st * nc + nc - 1]]))
    return out


HOT_PARTS = 6          # the hot file's hotword automata in six tests


@pytest.mark.parametrize("name,part", [(n, -1) for n in FILE_NAMES] + [(DC.HOT_FILE, k) for k in range(HOT_PARTS)])
def test_hot_run_against_re_search_on_every_slice(name, part, files):
    """every hotword automaton of the file against re.search(text[lo:hi]), hi - lo in 0 .. 70, at every lo of
    every row of the file.  (A slice equal to one already checked for the same automaton, as the rows' periodic
    filler gives many, is not checked twice.)"""
    _, comp, sim = files(name)
    rows = [r for _, r in _rows_of(name)]
    n_hit = n_seg = 0
    for h, hr in enumerate(comp.hot_rules):
        if part >= 0 and h % HOT_PARTS != part:
            continue
        rx = re.compile(hr.pattern.encode("ascii"))
        tables, seen = _hot_tables(sim, h), set()
        for t in rows:
            for lo in range(len(t) + 1):
                seg = t[lo:lo + 70]
                if seg in seen:
                    continue
                seen.add(seg)
                got = _hot_prefix_accepts(tables, seg)
                for n in range(len(seg) + 1):
                    assert got[n] == bool(rx.search(seg[:n])), (hr.pattern, t, lo, n)
                n_hit += sum(got)
                n_seg += 1
                if n_seg % 64 == 0:                # the one-pass form above is TableSim.hot_run
                    assert sim.hot_run(h, seg) == got[-1] and sim.hot_run(h, seg[:5]) == got[min(5, len(seg))]
    assert n_seg > 1000 and (n_hit > 0 or name != DC.HOT_FILE)


# --------------------------------------------------------------------------------------- whole rows
def _check_rows(sim, ocfg, comp, rows, variants):
    from oracle import pii_oracle as O
    groups = [t for t, _, _ in comp.rules.kw_groups]
    n = 0
    for label, t in rows:
        ev = sim.scan(t, True)
        for et in variants:
            v = 0 if et is None else 1 + groups.index(et)
            exp = [(f.start, f.end, f.type_id, f.likelihood) for f in O.find_pii(t, ocfg, et)]
            assert sim.resolve(t, ev, v) == exp, (label, t, et)
            n += len(exp)
    return n


@pytest.mark.parametrize("name", FILE_NAMES)
def test_whole_rows_against_the_oracle(name, files):
    """every row under variant 0, under the context variant of each custom type of the file and under two
    shipped types'"""
    ocfg, comp, sim = files(name)
    rows = DC.file_rows(name)
    variants = [None] + DC.own_types(name) + ["CVV_NUMBER", "MAC_ADDRESS"]
    assert _check_rows(sim, ocfg, comp, rows, variants) > 30 * len(DC.FILES[name])


@pytest.mark.parametrize("name", list(DC.HOT_COPIES))
def test_hot_rows_against_the_oracle(name, files):
    """HOT's context turns its first rule into fixed VERY_LIKELY, FW's appends the ".+" 100 / 100 rule"""
    ocfg, comp, sim = files(name)
    rows = _rows_of(name)
    assert _check_rows(sim, ocfg, comp, rows, [None] + DC.own_types(name)) > len(rows) // 8


def test_first_window_rows_against_the_oracle(files):
    from oracle import pii_oracle as O
    ocfg, comp, sim = files("hot")
    fw = DC.first_window_rows()
    _check_rows(sim, ocfg, comp, [(label, r) for label, r, _, _ in fw], [None] + DC.own_types("hot"))
    tid = ocfg.type_id["FW"]
    for label, row, s, n in fw:                       # the rows hold the match they are labelled with
        got = [(f.start, f.end) for f in O.find_pii(row, ocfg) if f.type_id == tid]
        assert got == ([(s, s + n)] if n > 0 else []), label


def test_lane_rows_against_the_oracle(files):
    from oracle import pii_oracle as O
    ocfg, comp, sim = files("hot")
    lane = DC.lane_rows()
    assert _check_rows(sim, ocfg, comp, lane, [None] + DC.own_types("hot")) > len(lane) // 2
    # the hotword decides in the lane rows too: both a lifted and an unlifted likelihood occur
    hid = ocfg.type_id["HOT"]
    assert len({f.likelihood for _, r in lane for f in O.find_pii(r, ocfg) if f.type_id == hid}) >= 3


# ------------------------------------------------------------------------------------------ the bug
def _custom_rules(patterns):
    comp = pkg("compiler")
    cfg, builtin = DC.rule_files()["lazy_any"]
    cfg["inspect_config"]["custom_info_types"] = [
        {"info_type": {"name": "T%d" % i}, "regex": {"pattern": p}, "likelihood": "LIKELY"}
        for i, p in enumerate(patterns)]
    return comp.Rules(cfg, builtin), cfg, builtin


def test_a_leading_optional_or_starred_group_compiles():
    r"""compile_rules rejected these ("relaxed pattern of ... can match the empty string"): relax_items ended the
    SCAN prefix at the optional group, before any required character"""
    import random
    from oracle import pii_oracle as O
    from tablesim import TableSim
    comp = pkg("compiler")
    pats = DC.FORMERLY_REJECTED + DC.REJECTED_IN_GROUP
    rules, cfg, builtin = _custom_rules(pats)
    c = comp.compile_rules(rules)
    sim, ocfg = TableSim(c), O.RuleConfig(cfg, builtin)
    rnd = random.Random(5)
    rows = [("r%d" % i, b"".join(rnd.choice(DC.REJECTED_FRAGS) for _ in range(rnd.randrange(1, 6))))
            for i in range(600)]
    assert _check_first_and_scan(sim, c, rows, ["T%d" % i for i in range(len(pats))]) > 10000
    assert _check_rows(sim, ocfg, c, rows, [None]) > 600
    for i in range(len(pats)):
        assert sum(f.type_id == ocfg.type_id["T%d" % i] for _, r in rows for f in O.find_pii(r, ocfg)) >= 30, i


def test_an_optional_group_that_ends_a_flag_group_is_still_refused():
    comp = pkg("compiler")
    for pat in DC.STILL_REFUSED:
        with pytest.raises(comp.RuleError, match="can match the empty string"):
            comp.compile_rules(_custom_rules([pat])[0])


@pytest.mark.parametrize("bad", [r"(?:ab)?", r"(?:ab)?\b", r"(?:ab)*(?:cd)?", r"a?(?:bc)*\B", r"a*", r"((?:ab)?)\b"])
def test_a_nullable_pattern_is_still_refused(bad):
    comp = pkg("compiler")
    with pytest.raises(comp.RuleError, match="can match the empty string"):
        comp.compile_rules(_custom_rules([bad])[0])
    with pytest.raises(comp.RuleError, match="can match the empty string"):
        comp.add_relaxed(comp.NFA(), bad, 0, 3, reverse=True)
