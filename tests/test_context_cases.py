"""The case lists of context_cases reach what they claim to (on the oracle alone), and the compiled keyword
automaton gives the oracle's group on every row of them (TableSim over the blob).  No GPU."""
import re

import pytest

import context_cases as CC
from conftest import pkg
from tablesim import TableSim


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    """rule file name -> (oracle RuleConfig, compiled rules)"""
    from oracle import pii_oracle as O
    comp = pkg("compiler")
    d = tmp_path_factory.mktemp("context")
    out = {}
    for name, pair in CC.rule_files().items():
        cfg, builtin = CC.write_rules(d, name, pair)
        out[name] = (O.RuleConfig.load(cfg, builtin), comp.compile_default(cfg, builtin))
    return out


def _first_group(name, text):
    """the lowest group with a keyword inside the ASCII-lowered text, by substring search over the lists of
    context_cases (not the oracle's code): (group index, type) or (None, miss type)"""
    low = bytes(c + 32 if 65 <= c <= 90 else c for c in text)
    hits = [g for g, _, k in CC.keywords_of(name) if k in low]
    if name == "kw":
        hits.append([t for t, _ in CC.KW_GROUPS].index(CC.ALWAYS_TYPE))
    if not hits:
        return None, None
    return min(hits), CC.groups_of(name)[min(hits)][0]


# ------------------------------------------------------------------------------------------ 1 reach
@pytest.mark.parametrize("name", CC.FILES)
def test_every_keyword_hits_in_its_three_casings(name, rules):
    """... its own group, unless it holds a keyword of an earlier group (shipped: "mac address" holds "address"),
    which then wins in all three casings alike"""
    from oracle import pii_oracle as O
    ocfg = rules[name][0]
    own = 0
    for g, t, k in CC.keywords_of(name):
        want = _first_group(name, k)
        assert want[0] is not None and want[0] <= g
        for v in (k, CC.upper(k), CC.mixed(k)):
            assert O.extract_expected_pii(v, ocfg) == want[1], (name, k, v)
        own += want[0] == g
    assert own >= (48 if name == "shipped" else 20)


@pytest.mark.parametrize("name", CC.FILES)
def test_groups_win_by_order_not_by_position(name, rules):
    """every group that can win at all (one of its keywords holds no keyword of an earlier group, and no always-hit
    group stands before it) wins a two-keyword row in which the other group's keyword stands earlier in the text;
    the others win no row of the list"""
    from oracle import pii_oracle as O
    ocfg = rules[name][0]
    groups = CC.groups_of(name)
    can_win = {g for g, t, k in CC.keywords_of(name) if _first_group(name, k)[0] == g}
    texts = CC.keyword_texts(name)
    won_late, won = set(), set()
    for label, text in texts:
        et = O.extract_expected_pii(text, ocfg)
        if et is not None:
            won.add([t for t, _ in groups].index(et))
        m = re.match(r"pair/(\d+)([<>])(\d+)", label)
        if m and et is not None:
            a, b = int(m.group(1)), int(m.group(3))
            late = b if m.group(2) == ">" else a          # "a>b": a's keyword first; "a<b": b's keyword first
            if groups[late][0] == et:
                won_late.add(late)
    live = sorted({g for g, _, _ in CC.keywords_of(name)})
    always = [t for t, _ in groups].index(CC.ALWAYS_TYPE) if name == "kw" else None
    # (against a keyword of a later group, so the file's last live group has no such row)
    assert won_late == {g for g in can_win if g < max(live)}, (sorted(won_late), sorted(can_win))
    assert won == can_win | ({always} if always is not None else set())
    assert len(can_win) >= (18 if name == "shipped" else 9) and set(live) - can_win       # both kinds exist
    if name == "kw":
        assert {g for g in live if g > always} and not {g for g in won if g > always}


@pytest.mark.parametrize("name", CC.FILES)
def test_near_misses_give_no_group(name, rules):
    from oracle import pii_oracle as O
    ocfg = rules[name][0]
    miss = CC.miss_type(name)
    n = 0
    for label, text in CC.keyword_texts(name):
        if label.split("/")[0].rstrip("0123456789") in ("del", "rep", "near", "glued", "odd-inside", "dropped"):
            n += O.extract_expected_pii(text, ocfg) == miss
    assert n >= 200, n
    if name == "kw":            # what an unescaped pattern, a folded É or a kept upper-case keyword would accept
        by = dict(CC.keyword_texts(name))
        for k, ns in CC.KW_NEAR.items():
            for i in range(len(ns)):
                assert O.extract_expected_pii(by["near/%s/%d" % (k, i)], ocfg) == miss, (k, i)
        for label in ("cafe-upper", "cafe-latin1", "ea-lower", "dropped/3", "dropped-lower/3", "dropped/13"):
            assert O.extract_expected_pii(by[label], ocfg) == miss, label
        assert O.extract_expected_pii(by["Ea-upper"], ocfg) == "IP_ADDRESS"
        assert O.extract_expected_pii(by["cafe-mixed"], ocfg) == "US_MEDICARE_BENEFICIARY_ID_NUMBER"     # "Café": C folds


# the issue's bound on the splits a half of which holds a whole keyword is 10 % of a file's splits.  The "kw"
# file's lists are chosen for it.  The shipped keywords cannot meet it -- "address" is the tail of seven other
# keywords, "drive" the head of two, "taxpayer id", "account number" and "passport no" lie inside longer ones --
# 137 of their 676 splits: that count is asserted exactly, so that a change of the lists is noticed, every dropped
# split is checked to hold a whole keyword, and all of them are still run on the GPU, where the oracle decides each.
SPLIT_DROP_LIMIT = {"kw": 0.10}
SPLIT_DROPPED = {"shipped": (137, 676)}


@pytest.mark.parametrize("name", CC.FILES)
def test_split_halves_give_no_group(name, rules):
    from oracle import pii_oracle as O
    ocfg = rules[name][0]
    miss = CC.miss_type(name)
    pairs = CC.split_pairs(name)
    assert len(pairs) == sum(len(k) - 1 for _, _, k in CC.keywords_of(name))
    dropped = 0
    for label, a, b in pairs:
        ea, eb = O.extract_expected_pii(a, ocfg), O.extract_expected_pii(b, ocfg)
        if ea == miss and eb == miss:
            continue
        dropped += 1
        assert any(k in a or k in b for _, _, k in CC.keywords_of(name)), label
    if name in SPLIT_DROPPED:
        assert (dropped, len(pairs)) == SPLIT_DROPPED[name]
    else:
        assert dropped <= SPLIT_DROP_LIMIT[name] * len(pairs), (dropped, len(pairs))
    assert len(pairs) - dropped >= 300


def _runs(rows):
    """[(first row, last row)] of the batch's runs"""
    out, a = [], 0
    for i in range(1, len(rows) + 1):
        if i == len(rows) or rows[i][0] != rows[a][0]:
            out.append((a, i - 1))
            a = i
    return out


def _facts(rows, ocfg, stored=()):
    """the run-structure conditions a batch holds, from its own columns"""
    from oracle import pii_oracle as O
    hit = {t: O.extract_expected_pii(t, ocfg) for t in {r[2] for r in rows}}
    have = set()
    stored = {sl: ts for sl, _g, ts in stored}
    for a, b in _runs(rows):
        have |= {("start", a), ("end", b)}
        if a == b:
            have.add("run of one")
        last, groups, missed = None, set(), False
        for i in range(a, b + 1):
            slot, role, text, ts = rows[i]
            et = hit[text]
            if role == CC.AGENT and et:
                if last is not None and hit[rows[last][2]] != et:
                    groups.add((hit[rows[last][2]], et))
                last, missed = i, False
                have.add("agent row's own group after a hit of another" if groups else "agent hit")
            elif role == CC.AGENT:
                missed = last is not None
            elif role == CC.CUSTOMER:
                if last is None:
                    have.add("customer before any hit")
                    if slot in stored:
                        have.add(("stored", ts - stored[slot] - CC.TTL_US))
                else:
                    have.add(("same run", ts - rows[last][3] - CC.TTL_US))
                    if ts < rows[last][3]:
                        have.add("timestamp lower than the hit's")
                    if groups:
                        have.add("customer after two hits of different groups")
                    if missed:
                        have.add("customer after a hit and a later miss")
            if role != CC.AGENT and et:
                have.add("keyword outside an agent row")
        if last is not None and rows[last][3] != rows[b][3]:
            have.add("hit's timestamp differs from the run's last row's")
        if last is None:
            have.add("run without a hit")
    return have


def test_run_structure_batches_hold_their_conditions(rules):
    from oracle import pii_oracle as O
    ocfg = rules[CC.RUN_FILE][0]
    assert ocfg.context_keywords == rules["shipped"][0].context_keywords
    for t, et in CC.HIT_TYPES.items():
        assert O.extract_expected_pii(t, ocfg) == et
    assert O.extract_expected_pii(CC.MISS, ocfg) is None and O.extract_expected_pii(CC.VALUE, ocfg) is None
    assert O.extract_expected_pii(CC.KWTXT, ocfg)
    assert not O.find_pii(CC.VALUE, ocfg) and not O.find_pii(CC.VALUE, ocfg, "US_SOCIAL_SECURITY_NUMBER")
    assert O.find_pii(CC.VALUE, ocfg, "CVV_NUMBER")                   # found only under its context
    rows = CC.edge_batch()
    assert 6100 <= len(rows) <= 6300 and max(len(r[2]) for r in rows) <= 20 and sum(len(r[2]) for r in rows) < 100_000
    have = _facts(rows, ocfg, CC.presets(rows, 0))
    for e in CC.EDGES:
        for d in (-1, 0, 1):
            assert ("start", e + d) in have and ("end", e + d) in have, (e, d)
    for cond in ("run of one", "agent row's own group after a hit of another", "customer before any hit",
                 "customer after two hits of different groups", "customer after a hit and a later miss",
                 "keyword outside an agent row", "run without a hit", "hit's timestamp differs from the run's last row's"):
        assert cond in have, cond
    # a run crosses a thread's, a wavefront's and a tile's last row with a hit before it and a customer after it
    hit = {t: O.extract_expected_pii(t, ocfg) for t in {r[2] for r in rows}}
    for step in (8, 512, 2048):
        assert any(a < m <= b and any(rows[i][1] == CC.AGENT and hit[rows[i][2]] for i in range(a, m)) and
                   any(rows[i][1] == CC.CUSTOMER for i in range(m, b + 1))
                   for a, b in _runs(rows) for m in range(step, len(rows), step)), step
    live = {d < 0 for c, d in (x for x in have if isinstance(x, tuple) and x[0] == "stored")}
    assert live == {True, False}                                     # presets live for some rows, expired for others
    # the long conversation and its sibling
    for sibling in (False, True):
        lb = CC.long_batch(sibling)
        runs = _runs(lb)
        assert len(lb) > 4100 and len(runs) == (2 if sibling else 1)
        hits = [i for i, r in enumerate(lb) if r[1] == CC.AGENT and O.extract_expected_pii(r[2], ocfg)]
        cust = [i for i, r in enumerate(lb) if r[1] == CC.CUSTOMER]
        assert hits == [1] and cust and min(cust) >= 4096 and max(cust) < 6144
        if sibling:
            assert 2048 < runs[1][0] < 4096
    # the timestamps of the TTL batch
    one, two = CC.ttl_batch()
    pre = [(CC.slot_of(10 + k), 0, CC.T0) for k in range(3)]
    h1 = _facts(one, ocfg, pre)
    for d in (-1, 0, 1):
        assert ("same run", d) in h1 and ("stored", d) in h1, d
    assert "timestamp lower than the hit's" in h1 and "hit's timestamp differs from the run's last row's" in h1
    store = O.ContextStore()
    for sl, _g, ts in pre:
        store.set(sl, "CVV_NUMBER", b"", ts)
    O.process_rows(one, ocfg, store)
    after = {sl: v[2] for sl, v in store.d.items()}
    deltas = {r[3] - after[r[0]] - CC.TTL_US for r in two if r[1] == CC.CUSTOMER and _runs(two) and r[0] in after}
    assert {-1, 0, 1} <= deltas                                      # ... after a record an earlier call stored


# --------------------------------------------------------------------------------------- 2 the compiler
def test_kw_file_compiles_to_the_expected_groups(rules):
    ocfg, comp = rules["kw"]
    got = comp.rules.kw_groups[:comp.rules.n_keyword_groups]
    assert comp.rules.n_keyword_groups == len(CC.KW_GROUPS)
    for (t, pat, always), (wt, wk, wa) in zip(got, CC.KW_COMPILED):
        assert t == wt and always == wa
        assert pat == (b"(?i)(?:" + b"|".join(re.escape(k) for k in wk) + b")" if wk else None), t
    by = {t: (wk, wa) for t, wk, wa in CC.KW_COMPILED}
    assert by["EMAIL_ADDRESS"] == ([], False) and by["DATE_OF_BIRTH"] == ([], False) and by["STREET_ADDRESS"] == ([], False)
    assert by[CC.ALWAYS_TYPE] == ([b"zulu"], True) and by["FINANCIAL_ACCOUNT_NUMBER"][0] == [b"911", b"~"]
    assert by["IP_ADDRESS"][0] == [b"dup word", "Éa".encode("utf-8")]
    always = [int(x) for x in comp.sections["kw.always"][:len(CC.KW_GROUPS)]]
    assert always == [1 if wa else 0 for _, _, wa in CC.KW_COMPILED] and sum(always) == 1
    # the engine and the oracle number the types alike (the GPU tests compare info_type numbers)
    assert list(comp.rules.type_names) == list(ocfg.type_names)
    assert list(rules["shipped"][1].rules.type_names) == list(rules["shipped"][0].type_names)


def test_group_order_is_part_of_the_compile_cache_key(tmp_path):
    """two rule files that differ in the order of their context_keywords groups alone compile to two blobs"""
    import yaml
    comp = pkg("compiler")
    cfg, builtin = CC.rule_files()["shipped"]
    kws = cfg["context_keywords"]
    paths = []
    for tag, order in (("fwd", list(kws)), ("rev", list(kws)[::-1])):
        c = dict(cfg, context_keywords={t: kws[t] for t in order})
        p = tmp_path / (tag + ".yaml")
        p.write_text(yaml.safe_dump(c, sort_keys=False))
        paths.append(str(p))
    bp = tmp_path / "builtin.yaml"
    bp.write_text(yaml.safe_dump(builtin))
    a, b = (comp.compile_default(p, str(bp)) for p in paths)
    assert [t for t, _, _ in a.rules.kw_groups[:3]] != [t for t, _, _ in b.rules.kw_groups[:3]]
    assert a.blob != b.blob


def _kw_scan(sim):
    """TableSim's reverse K scan and keyword_group for AGENT rows, on the K tables alone (the D automaton decides
    nothing here): the same table walk, without the per-byte D step, so that the lane rows' 3 MB take seconds"""
    cm = [int(x) >> 8 for x in sim.cmap2]
    tk = [[int(x) for x in row] for row in sim.tk]
    kacc = [[int(x) for x in row] for row in sim.kacc]
    k_off, k_ids = [int(x) for x in sim.k_off], [int(x) for x in sim.k_ids]
    base = min([g for g in range(sim.G) if sim.kw_always[g]] or [1 << 30])
    eot = sim.CK - 1

    def group(text):
        best, sk = base, sim.k_start
        for j in range(len(text) - 1, -1, -1):
            c = cm[text[j]]
            nk = tk[sk][c]
            if nk & 0x8000:                                  # event at j + 1: the class of the byte before it is c
                a = kacc[sk][c]
                for i in range(k_off[a], k_off[a + 1]):
                    best = min(best, k_ids[i])
            sk = nk & 0x7FFF
        if tk[sk][eot] & 0x8000:
            a = kacc[sk][eot]
            for i in range(k_off[a], k_off[a + 1]):
                best = min(best, k_ids[i])
        return -1 if best == 1 << 30 else best
    return group


@pytest.mark.parametrize("name", CC.FILES)
def test_compiled_keyword_automaton_equals_the_oracle(name, rules):
    from oracle import pii_oracle as O
    ocfg, comp = rules[name]
    sim = TableSim(comp)
    groups = [t for t, _, _ in comp.rules.kw_groups]
    texts = [t for _, t in CC.keyword_texts(name)]
    for _, a, b in CC.split_pairs(name):
        texts += [a, b]
    fast = _kw_scan(sim)
    hits = 0
    for text in texts:
        kg = sim.keyword_group(text, sim.scan(text, True))
        assert kg == fast(text), text
        et = O.extract_expected_pii(text, ocfg)
        assert (groups[kg] if kg >= 0 else None) == et, text
        hits += et != CC.miss_type(name)
    assert hits > 500
    lane, where = CC.lane_rows(name)
    whole = 0
    for (label, row), (_, c, j) in zip(lane, where):
        kg = fast(row)
        et = O.extract_expected_pii(row, ocfg)
        assert (groups[kg] if kg >= 0 else None) == et, label
        whole += et != CC.miss_type(name)
    assert len(lane) // 3 < whole < 2 * len(lane) // 3 + 50        # the rows hit, (most of) their siblings do not


@pytest.mark.parametrize("name", CC.FILES)
@pytest.mark.parametrize("r0", [0, 7, 48])
def test_lane_rows_put_every_split_on_a_cut(name, r0):
    """the geometry the rows were built for, recomputed from the packed batch: a row of more than 256 bytes is cut
    where (batch position + r0) is a multiple of 128"""
    every = 1
    lane, where = CC.lane_rows(name, r0=r0, every=every)
    pos, seen, two_cuts = 0, set(), 0
    for (label, row), (i, c, j) in zip(lane, where):
        assert 300 <= len(row) <= 700
        assert (pos + c + r0) % 128 == 0 and 0 < c < len(row), label
        g, k = next((g, k) for g, _, k in CC.keywords_of(name) if label.split("/")[2] == str(g) and
                    label.split("/")[3] == k[:12].decode("latin-1") and len(k) > j)
        if not label.endswith("/sib"):
            assert row[c - j:c - j + len(k)] == k, label
            seen.add((k, j, label.split("/")[1]))
            two_cuts += sum(1 for x in CC.lane_cuts(pos, len(row), r0, 128) if c - j < x < c - j + len(k)) >= 2
        pos += len(row)
    want = {(k, j) for _, _, k in CC.keywords_of(name) for j in range(1, len(k), every)}
    assert {(k, j) for k, j, _ in seen} == want and {w for _, _, w in seen} == {"first", "mid", "last"}
    assert (two_cuts > 10) == (name == "kw")                      # the 140-byte keyword across two cuts
    assert pos < (16 << 20)                                       # a batch this small gets 128-byte lanes
