"""The regex dialect and the hotword geometry on the GPU: a user's regexes reach k_scan, k_pair_first
(first_begin / first_finish), k_pair_eval (hot_run, hot_rule_apply) and the window kernels (k_win_eval,
k_win_halo, k_win_lik, k_win_select; hot_span_pre, hot_run_joined) as automata compiled from them.  The case
lists of dialect_cases -- 49 detector patterns over nine rule files, the hotword rule file with every window size
around the runners' 4-, 16- and 64-byte steps, the first-window, hotword and lane rows -- run through the host
and device entry points, the batch path's long rows and the window path's three modes.

Every row of every list is compared with the oracle on the same rows -- spans (utt, start, end, info_type,
likelihood), output bytes, offsets and the histogram; none is sampled or skipped, under no context and under
the context of each of the file's own types.  The window test builds conversations of its own from the files'
rows.  test_dialect_cases.py (no GPU) checks that the lists reach what they
claim to.  Needs an MI355X: pytest -m gpu."""
import os

import numpy as np
import pytest

import dialect_cases as DC
from conftest import pkg
from test_gpu_validators import _check_device, _check_host, _spans_of

pytestmark = pytest.mark.gpu

FILE_NAMES = list(DC.FILES)


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    """rule file name -> (oracle RuleConfig, compiled rules)"""
    from oracle import pii_oracle as O
    comp = pkg("compiler")
    d = tmp_path_factory.mktemp("dialect")
    out = {}
    for name, pair in DC.rule_files().items():
        cfg, builtin = DC.write_rules(d, name, pair)
        out[name] = (O.RuleConfig.load(cfg, builtin), comp.compile_default(cfg, builtin))
    return out


@pytest.fixture(scope="module")
def engines(rules):
    E = pkg("engine")
    made = {}

    def get(name):
        if name not in made:
            made[name] = E.Engine(rules[name][1].blob, device=0, n_conv_slots=1 << 12)
        return made[name]
    yield get
    for e in made.values():
        e.close()


def _check_host_context(eng, texts, ocfg, expected_type, labels):
    """customer rows, one conversation each, the context preset with pii_context_set to `expected_type`: the
    same comparison as _check_host"""
    from oracle import pii_oracle as O
    assert len(texts) <= 1 << 12
    g = eng.group_types.index(expected_type)
    store = O.ContextStore()
    rows = []
    for i, t in enumerate(texts):
        eng.context_set(i, g, 1_000_000)
        store.set(i, expected_type, b"", 1_000_000)
        rows.append((i, O.ROLE_CUSTOMER, t, 1_000_001))
    exp = O.process_rows(rows, ocfg, store)
    assert all(x[2] == expected_type for x in exp)
    eng.histogram_reset()
    res = eng.scan_redact(texts, [r[0] for r in rows], [r[1] for r in rows], [r[3] for r in rows])
    for i, x in enumerate(exp):
        assert res.text(i) == x[0], (labels[i], expected_type, texts[i], res.text(i), x[0])
    assert [int(o) for o in res.out_offsets] == [0] + list(np.cumsum([len(x[0]) for x in exp]))
    got = [(int(s["utt"]), int(s["start"]), int(s["end"]), int(s["info_type"]), int(s["likelihood"]))
           for s in res.spans]
    assert got == _spans_of(exp)
    hist = eng.histogram()
    assert (hist == np.bincount(res.spans["info_type"].astype(np.int64), minlength=len(hist))[:len(hist)]).all()
    for i in range(len(texts)):
        eng.context_set(i, -1, 0)
    return exp


def _count(exp, ocfg, t):
    return sum(f.type_id == ocfg.type_id[t] for x in exp for f in x[1])


# ------------------------------------------------------------------------------- 1 the dialect files
@pytest.mark.parametrize("name", FILE_NAMES)
def test_dialect_rows_on_the_host_path(name, rules, engines):
    ocfg = rules[name][0]
    rows = DC.file_rows(name)
    exp = _check_host(engines(name), [r for _, r in rows], ocfg, [label for label, _ in rows])
    for t in DC.own_types(name):
        assert _count(exp, ocfg, t) >= 30, t


@pytest.mark.parametrize("name", FILE_NAMES)
def test_dialect_rows_under_each_types_context(name, rules, engines):
    ocfg, eng = rules[name][0], engines(name)
    rows = DC.file_rows(name)
    for t in DC.own_types(name):
        _check_host_context(eng, [r for _, r in rows], ocfg, t, [label for label, _ in rows])


def _interleaved(lists):
    """row k from list k % len(lists), each list cycled with a step coprime to its length: neighbouring rows
    (and neighbouring pairs of k_pair_first) hold different patterns"""
    steps = [next(p for p in (37, 41, 43, 47, 53) if len(rows) % p) for rows in lists]
    n = max(len(rows) for rows in lists)
    return [rows[(i * step) % len(rows)] for i in range(n) for rows, step in zip(lists, steps)]


@pytest.mark.parametrize("name", [n for n in FILE_NAMES if len(DC.FILES[n]) > 1])
def test_interleaved_patterns_share_a_wavefront(name, rules, engines):
    ocfg = rules[name][0]
    rows = _interleaved([[("%s/%d" % (p["name"], i), r) for i, r in enumerate(DC.pattern_rows(p))]
                         for p in DC.FILES[name]])
    exp = _check_host(engines(name), [r for _, r in rows], ocfg, [label for label, _ in rows])
    for t in DC.own_types(name):
        assert _count(exp, ocfg, t) >= 30, t


def test_interleaved_short_and_continued_first_runs(rules, engines):
    """matches that end in first_begin's window beside matches first_finish continues, hotword rows between
    them: k_pair_first's `cont` queue and its `matched` queue both fill in one workgroup"""
    ocfg = rules["hot"][0]
    fw = DC.first_window_rows()
    short = [(label, r) for label, r, s, n in fw if n <= 14]
    long_ = [(label, r) for label, r, s, n in fw if n >= 17]
    hot = [(label, r) for label, r, *_ in DC.hot_rows()]
    rows = _interleaved([short, long_, hot])
    exp = _check_host(engines("hot"), [r for _, r in rows], ocfg, [label for label, _ in rows])
    assert _count(exp, ocfg, "FW") > len(rows) // 3 and _count(exp, ocfg, "HOT") > 100


# ------------------------------------------------------------------- 2 the runners' geometry, device
def test_first_window_rows_on_the_device_path(rules, engines):
    ocfg = rules["hot"][0]
    fw = DC.first_window_rows()
    exp, _ = _check_device(engines("hot"), [r for _, r, _, _ in fw], ocfg, [label for label, _, _, _ in fw])
    tid = ocfg.type_id["FW"]
    for (label, row, s, n), x in zip(fw, exp):
        assert [(f.start, f.end) for f in x[1] if f.type_id == tid] == ([(s, s + n)] if n > 0 else []), label


def test_hot_rows_on_the_device_path(rules, engines):
    ocfg = rules["hot"][0]
    hot = DC.hot_rows()
    exp, _ = _check_device(engines("hot"), [r for _, r, *_ in hot], ocfg, [label for label, *_ in hot])
    hid = ocfg.type_id["HOT"]
    assert {f.likelihood for x in exp for f in x[1] if f.type_id == hid} == {3, 4, 5}


@pytest.mark.parametrize("name", list(DC.HOT_COPIES))
def test_hot_rows_under_each_min_likelihood(name, rules, engines):
    ocfg, eng = rules[name][0], engines(name)
    hot = DC.hot_rows()
    texts, labels = [r for _, r, *_ in hot], [label for label, *_ in hot]
    exp = _check_host(eng, texts, ocfg, labels)
    liks = {f.likelihood for x in exp for f in x[1] if f.type_id == ocfg.type_id["HOT"]}
    assert liks == {"hot": {3, 4, 5}, "hot_likely": {4, 5}, "hot_very_unlikely": {1, 2, 3, 4, 5}}[name]
    fw = DC.first_window_rows()
    for t in DC.own_types(name):                      # HOT: its first rule fixed VERY_LIKELY; FW: the ".+" rule
        _check_host_context(eng, texts, ocfg, t, labels)
        for a in range(0, len(fw), 1 << 12):          # one conversation slot per row: 4096 rows a call
            part = fw[a:a + (1 << 12)]
            _check_host_context(eng, [r for _, r, _, _ in part], ocfg, t, [label for label, _, _, _ in part])


def test_lane_rows_on_the_batch_path(rules, engines):
    ocfg = rules["hot"][0]
    lane = DC.lane_rows()
    exp = _check_host(engines("hot"), [r for _, r in lane], ocfg, [label for label, _ in lane])
    hid = ocfg.type_id["HOT"]
    assert len({f.likelihood for x in exp for f in x[1] if f.type_id == hid}) >= 3
    _check_device(engines("hot"), [r for _, r in lane], ocfg, [label for label, _ in lane])


# ----------------------------------------------------------------------------------- 3 the window path
def _hot_conversations():
    """conversations of seven rows (the window holds five).  Row 1 ends with a hotword of HOT's rule k, g bytes
    before its end; row 2 holds the match at offset o = 0 .. 3, so the hotword is g + 1 + o bytes before it, the
    "\\n" of the join between them (hot_run_joined); row 3 holds another rule's hotword g2 bytes in, within or
    just outside window_after of row 2's match; rows 5 and 6 repeat the pair with the match at offset 0."""
    convs = []
    for k, (text, _rx, w, _fx, _rel) in enumerate(DC.HOT_RULES):
        k2 = (k + 5) % len(DC.HOT_RULES)
        text2, w2 = DC.HOT_RULES[k2][0], DC.HOT_RULES[k2][2]
        for o in range(4):
            for g in sorted({0, max(0, w - len(text) - 1 - o), max(0, w - len(text) - o)}):
                o2 = (o + k) % 3
                g2 = max(0, w2 - len(text2) - 1 - o2 - (g & 1))
                convs.append([
                    DC.fill(5, k) + b"x",
                    DC.fill(3, o) + text + DC.fill(g, 1),
                    DC.fill(o, 2) + DC.HOT_MATCH + DC.fill(o2, 3),
                    DC.fill(g2, 4) + text2 + DC.fill(2, 5),
                    DC.ORD_MATCH + DC.fill(1, 0) + b"ob oc",
                    b"oa" + DC.fill(2, 1) + text + DC.fill(g, 2),
                    DC.HOT_MATCH,
                ])
    # a before-window's part inside the previous utterance of 65 .. 80 bytes, the hotword in its bytes past 64
    # (hot_span_pre loads four chunks of 16 and hands longer spans to hot_span)
    text = DC.HOT_RULES[-1][0]
    assert DC.HOT_RULES[-1][2] == 300
    for n in (65, 66, 70, 79, 80, 81):
        for o in range(4):
            prev = DC.fill(n - len(text) - (o & 1), o) + text + DC.fill(o & 1, 1)
            convs.append([b"x", prev, DC.fill(o, 2) + DC.HOT_MATCH, b"y", prev + b";", DC.HOT_MATCH, b"z"])
    return convs


def _file_conversations(name):
    rows = [r.replace(b"\n", b"|") for _, r in DC.file_rows(name)]         # "\n" is the window's join
    convs = [rows[i:i + 7] for i in range(0, len(rows) - 6, 7)]
    if name == DC.LIFTED["REP_PLUS_LAZY"]["file"]:
        # the lifting hotword at the end of the previous utterance, the match at offsets 0 .. 3 of the next
        for o in range(4):
            convs.append([b"x", b"say KEY", b" " * o + b"f12g", b"KEY", b"f1g f7", b"the KEY ", b"f123g KEY"])
    return convs


@pytest.mark.parametrize("name", DC.WINDOW_FILES)
def test_window_rescan_whole_cut_and_full(name, rules):
    """rows whole, rows cut at every scan lane (PII_WIN_LONG=1, read when the engine is created) and the full
    re-scan give the oracle's windows, and one another's"""
    from oracle import pii_oracle as O
    E = pkg("engine")
    ocfg, comp = rules[name]
    assert int(comp.sections["meta"][13]) == 1          # no detector of the file consumes "\n" or tests a text edge
    convs = _hot_conversations() if name == DC.HOT_FILE else _file_conversations(name)
    modes = [("incremental", {}), ("incremental", {"PII_WIN_LONG": "1"}), ("full", {})]
    convs = [[(c + 1, k & 1, t, 10 + k) for k, t in enumerate(conv)] for c, conv in enumerate(convs)]
    assert 30 <= len(convs) <= 1000
    made = []
    try:
        for mode, env in modes:
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                eng = E.Engine(comp.blob, device=0, n_conv_slots=1024)
            finally:
                for k, v in old.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
            made.append(eng)
            eng.window_enable(5, 8192, full=mode == "full")
            assert eng.window_mode() == mode
        store, hist = O.ContextStore(), {}
        found, liks = 0, set()
        for k in range(7):
            batch = [conv[k] for conv in convs]
            args = ([r[2] for r in batch], [r[0] for r in batch], [r[1] for r in batch], [r[3] for r in batch])
            got = [eng.rescan_window(*args) for eng in made]
            exp = O.process_window_rows(batch, ocfg, n=5, store=store, history=hist)
            for i, (red, fs, _) in enumerate(exp):
                for res in got:
                    assert res.text(i) == red, (k, i, batch[i])
                    m = res.spans["utt"] == i
                    assert [(int(s["start"]), int(s["end"]), int(s["info_type"]), int(s["likelihood"]))
                            for s in res.spans[m]] == [(f.start, f.end, f.type_id, f.likelihood) for f in fs]
                assert len({res.text(i) for res in got}) == 1              # incremental = cut = full re-scan
                found += len(fs)
                liks |= {f.likelihood for f in fs}
        assert found > 5 * len(convs)
        if name == DC.HOT_FILE:
            assert liks == {3, 4, 5}
    finally:
        for eng in made:
            eng.close()
