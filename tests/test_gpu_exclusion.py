"""General exclusion rules on the GPU (k_exclude) against the oracle: PARTIAL_MATCH, more excluder
patterns than k_select's streaming form holds, a type both excluded and excluding (excl_configs G1 / G2 /
G3).  Rows, templates and the count of exclusions by shape: excl_rows.  Needs an MI355X: pytest -m gpu."""
import ctypes

import numpy as np
import pytest

import excl_configs as XC
import excl_rows as XR
import xform_ref
from conftest import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cfgs(tmp_path_factory):
    """name -> (config dict, compiled rules, the oracle's view of it)"""
    from oracle import pii_oracle as O
    comp = pkg("compiler")
    d = tmp_path_factory.mktemp("excl")
    out = {}
    for name, make in XC.CONFIGS.items():
        cfg = make()
        path = XC.write(d, name, cfg)
        out[name] = (cfg, comp.compile_default(path), O.RuleConfig.load(path))
    return out


@pytest.fixture(scope="module")
def engines(cfgs):
    E = pkg("engine")
    made = {}

    def get(name):
        if name not in made:
            made[name] = E.Engine(cfgs[name][1].blob, device=0, n_conv_slots=1 << 12)
        return made[name]
    yield get
    for e in made.values():
        e.close()


def _spans(res):
    return [(int(s["utt"]), int(s["start"]), int(s["end"]), int(s["info_type"]), int(s["likelihood"])) for s in res.spans]


def _check(eng, rows, exp, want):
    """one host call: every row's bytes, the offsets, the spans and the histogram, bit-exact"""
    eng.histogram_reset()
    res = eng.scan_redact([r[2] for r in rows], [r[0] for r in rows], [r[1] for r in rows], [r[3] for r in rows])
    for i, w in enumerate(want):
        assert res.text(i) == w, (i, rows[i][2][:120], res.text(i)[:120], w[:120])
    assert [int(o) for o in res.out_offsets] == [0] + [int(x) for x in np.cumsum([len(w) for w in want])]
    assert _spans(res) == [(i, f.start, f.end, f.type_id, f.likelihood) for i, x in enumerate(exp) for f in x[1]]
    hist = eng.histogram()
    assert (hist == np.bincount(res.spans["info_type"].astype(np.int64), minlength=len(hist))[:len(hist)]).all()
    return res


def _other(texts):
    from oracle import pii_oracle as O
    return [(0, O.ROLE_OTHER, t, 0) for t in texts]


# --------------------------------------------------------------------------------- 1 known answers
def test_known_answers(cfgs, engines, compiled):
    from oracle import pii_oracle as O
    E = pkg("engine")
    eng = engines("G1")
    assert eng.exclusion_mode() == 1
    rows = _other([t for t, _, _ in XC.KNOWN_G1])
    exp = O.process_rows(rows, cfgs["G1"][2])
    res = _check(eng, rows, exp, [x[0] for x in exp])
    names = eng.type_names
    for i, (text, want, _) in enumerate(XC.KNOWN_G1):
        assert res.text(i) == want
    got = [(u, s, e, names[t]) for u, s, e, t, _ in _spans(res)]
    assert got == [(0, 6, 15, "OUR_DOMAIN"), (1, 2, 15, "EMAIL_ADDRESS"), (2, 0, 11, "US_SOCIAL_SECURITY_NUMBER"),
                   (3, 0, 7, "PAIR3"), (3, 8, 19, "US_SOCIAL_SECURITY_NUMBER"), (4, 5, 24, "TEST_CARD")]
    shipped = E.Engine(compiled.blob, device=0, n_conv_slots=16)
    try:
        assert shipped.exclusion_mode() == 0
    finally:
        shipped.close()


# ----------------------------------------------------------------------------------------- 2 parity
# G2's entries are all FULL_MATCH: an excluder can only contain its victim, and no excluder type is excluded
NEEDED = {"G1": XR.SHAPES, "G2": ("contained",)}


@pytest.mark.parametrize("name", ["G1", "G2"])
def test_parity_every_context_variant(name, cfgs, engines):
    from oracle import pii_oracle as O
    eng, ocfg = engines(name), cfgs[name][2]
    assert eng.exclusion_mode() == 1
    groups = eng.group_types
    rows, contexts = XR.parity_rows(groups)
    assert len({r[0] for r in rows}) == 1 + len(groups)          # no context + every context group
    for slot, g in contexts.items():
        eng.context_set(slot, g, 0)
    exp = O.process_rows(rows, ocfg, XR.oracle_store(contexts, groups))
    assert [x[2] for x in exp] == [groups[contexts[r[0]]] if r[0] else None for r in rows]
    counts = XR.shape_counts(rows, exp, ocfg)
    print(name, len(rows), "rows; rows with an exclusion by shape:", counts)
    for s in NEEDED[name]:
        assert counts[s] >= 20, (s, counts)
    _check(eng, rows, exp, [x[0] for x in exp])


# --------------------------------------------------------------------------------------- 3 cut rows
def test_cut_rows(cfgs, engines):
    from oracle import pii_oracle as O
    eng, ocfg = engines("G1"), cfgs["G1"][2]
    texts = XR.cut_rows()
    assert len(texts) <= 200 and all(500 <= len(t) <= 700 for t in texts)
    rows = _other(texts)
    exp = O.process_rows(rows, ocfg)
    fired = sum(1 for t in texts if XR.exclusion_shapes(t, ocfg, None))
    assert fired >= 128                                          # (the e-mail and TAIL_REF snippets exclude; the PAIR3 one must not)
    _check(eng, rows, exp, [x[0] for x in exp])
    st = eng.stats(gate=True)
    assert st["lane_bytes"] == 128 and st["cut_rows"] == len(texts)


# ------------------------------------------------------------------------------------------- 4 G3
def test_allow_list_with_kept_types(cfgs, engines):
    from oracle import pii_oracle as O
    cfg, _, ocfg = cfgs["G3"]
    eng = engines("G3")
    assert eng.exclusion_mode() == 1
    import random
    r = random.Random(9)
    texts = [t for t, _, _ in XC.KNOWN_G1] + XR.template_texts(r, 400)
    rows = _other(texts)
    exp = O.process_rows(rows, ocfg)
    want = [xform_ref.apply_transform(t, x[1], ocfg.type_names, cfg) for t, x in zip(texts, exp)]
    res = _check(eng, rows, exp, want)
    # the allow-listed address, reference and test card come out as they went in
    assert res.text(0) == b"x jane@acme.com y" and res.text(1) == b"x [EMAIL_ADDRESS] y"
    assert res.text(2) == b"[US_SOCIAL_SECURITY_NUMBER] #212-555-0187 ok"
    assert res.text(4) == b"card 4111 1111 1111 1111 ok"


# --------------------------------------------------------------------------------------- 5 window
def test_window_rescan_is_full_and_exact(cfgs):
    from oracle import pii_oracle as O
    import random
    E = pkg("engine")
    _, c, ocfg = cfgs["G1"]
    r = random.Random(13)
    synth = pkg("synth")
    bank = synth.build_bank(50, 300, seed=13).texts
    C = O.ROLE_CUSTOMER
    rows = []
    for conv in range(200):
        for k in range(8):
            x = r.random()
            if conv == 0:      # excluder and victim in one utterance, the utterance between two "\n" joins
                t = [b"hello", b"jane@acme.com", b"ok", b"536-22-1234 #212-555-0187", b"bye", b"@acme.com",
                     b"bob@acme.org", b"4111 1111 1111 1111"][k]
            elif x < 0.6:
                t = XR.template_texts(r, 1)[0]
            else:
                t = r.choice(bank)
            rows.append((conv, C, t, 1 + k))
    eng = E.Engine(c.blob, device=0, n_conv_slots=256)
    try:
        eng.window_enable(5, 8192)
        assert eng.window_mode() == "full" and eng.exclusion_mode() == 1
        res = eng.rescan_window([t for _, _, t, _ in rows], [s for s, _, _, _ in rows], [x for _, x, _, _ in rows],
                                [s for _, _, _, s in rows])
        exp = O.process_window_rows(rows, ocfg, n=5)
        assert exp[1][0] == b"hello\njane[OUR_DOMAIN]" and exp[3][0].endswith(b"\n[US_SOCIAL_SECURITY_NUMBER] #212-555-0187")
        by_row = {}
        for s in res.spans:
            by_row.setdefault(int(s["utt"]), []).append((int(s["start"]), int(s["end"]), int(s["info_type"]),
                                                         int(s["likelihood"])))
        for i, (red, fs, _) in enumerate(exp):
            assert res.text(i) == red, (i, rows[i], res.text(i), red)
            assert by_row.get(i, []) == [(f.start, f.end, f.type_id, f.likelihood) for f in fs], (i, rows[i])
    finally:
        eng.close()


# --------------------------------------------------------------------------------------- 6 re-runs
def test_capacity_rerun(cfgs, engines):
    """a call whose output and span capacities are too small fails with PII_E_CAPACITY and names the need; the
    call repeated with it gives the oracle's output"""
    from oracle import pii_oracle as O
    E = pkg("engine")
    eng, ocfg = engines("G1"), cfgs["G1"][2]
    import random
    texts = XR.template_texts(random.Random(21), 300)
    rows = _other(texts)
    exp = O.process_rows(rows, ocfg)
    data, offs = E.pack(texts)
    n = len(texts)
    slot, role, ts = np.zeros(n, np.uint32), np.full(n, O.ROLE_OTHER, np.uint8), np.zeros(n, np.int64)

    def call(out_cap, span_cap):
        out, oo = np.empty(out_cap, np.uint8), np.zeros(n + 1, np.uint64)
        sp, ns, ctx = np.empty(span_cap, E.SPAN_DTYPE), ctypes.c_uint32(0), np.empty(n, np.int16)
        rc = eng.lib.pii_scan_redact(eng.h, E._ptr(data), E._ptr(offs), n, E._ptr(slot), E._ptr(role), E._ptr(ts),
                                     E._ptr(out), out_cap, E._ptr(oo), E._ptr(sp), span_cap, ctypes.byref(ns), E._ptr(ctx))
        return rc, out, oo, sp, int(ns.value)
    rc, _, oo, _, ns = call(64, 4)
    want = [x[0] for x in exp]
    assert rc == E.PII_E_CAPACITY
    assert int(oo[-1]) == sum(len(w) for w in want) and ns == sum(len(x[1]) for x in exp)
    rc, out, oo, sp, ns2 = call(int(oo[-1]) + 64, ns + 16)
    assert rc == E.PII_OK and ns2 == ns
    res = E.BatchResult(out[:int(oo[-1])], oo, sp[:ns2].copy(), None)
    for i, w in enumerate(want):
        assert res.text(i) == w, (i, texts[i])
    assert _spans(res) == [(i, f.start, f.end, f.type_id, f.likelihood) for i, x in enumerate(exp) for f in x[1]]


def test_queue_reruns(cfgs):
    """rows dense with allow-list matches overflow the occurrence list's first sizing (one per 64 bytes), rows
    dense with candidates the pair queue's (one per 16 bytes): pii_sync grows the list and runs the call
    again, with the oracle's output"""
    from oracle import pii_oracle as O
    E = pkg("engine")
    _, c, ocfg = cfgs["G1"]
    import random
    # 255-byte rows (not cut): 8 occurrences (4 e-mails, 4 OUR_DOMAIN) and 12 candidate pairs each -- 20800
    # occurrences against a first sizing of 14455, 31200 pairs against 45533
    snip = b"a@acme.com " + b"lorem ipsum dolor sit amet consectetur adipiscing elit"[:52] + b" "
    dense_occ = [(snip * 4)[:255]] * 2600
    r = random.Random(77)
    dense_pairs = [" ".join("".join(r.choice("0123456789-") for _ in range(r.randint(3, 19))) for _ in range(12)).encode()
                   + b" bob@example.com" for _ in range(600)]
    for name, texts in (("occurrences", dense_occ), ("pairs", dense_pairs)):
        eng = E.Engine(c.blob, device=0, n_conv_slots=16)                     # fresh: the queues at their first sizing
        try:
            rows = _other(texts)
            memo = {}
            exp = [memo.get(t) or memo.setdefault(t, O.process_rows([row], ocfg)[0]) for row, t in zip(rows, texts)]
            res = eng.scan_redact(texts, [0] * len(texts), [O.ROLE_OTHER] * len(texts), [0] * len(texts))
            st = eng.stats(gate=True)
            first = sum(len(t) for t in texts) // 16 + 4096                   # the pair queue's first sizing
            print(name, st, "pair queue first sized", first)
            assert st["cut_rows"] == 0
            if name == "occurrences":
                assert st["pairs"] <= first and st["reruns"] == 1, st         # only the occurrence list overflowed
            else:
                assert st["pairs"] > first and st["reruns"] >= 1, st
            for i, x in enumerate(exp):
                assert res.text(i) == x[0], (name, i)
            assert _spans(res) == [(i, f.start, f.end, f.type_id, f.likelihood) for i, x in enumerate(exp) for f in x[1]]
        finally:
            eng.close()
