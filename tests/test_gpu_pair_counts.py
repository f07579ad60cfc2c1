"""Pair counts at the source: the scan kernels (k_scan, and k_scan_fix's re-scan of a cut lane)
write each lane's (start, pattern) pair count next to its event count, the count pass
k_pairs_flat<false> is not launched, and the write pass records the AGENT rows' keyword groups.
PII_SCAN_COUNT=0 restores the count pass.  Nothing a caller sees may change: on the smallest shapes
where the new producer can go wrong (128-byte lanes), both forms agree bit for bit with each other
(output bytes, out_offsets, spans, per-row context, histogram, queue sizes) and with the oracle.
"""
import functools
import os
import random

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

LANE = 128
FILL = b"please note that the shipment will arrive on monday morning before noon at the usual place "
# AGENT rows whose only scan events are keyword hits (no D accept: checked with TableSim below)
KW_ONLY = [b"please tell me the cvv on the card", b"what is your social security number",
           b"could you read me the card number please", b"what is your email address?",
           b"may i have your phone number"]
VALUES = [b"sure it is 123", b"it is 536-22-8726", b"4111 1111 1111 1111", b"jane.doe@example.com",
          b"(415) 555-0132"]


def _engine(blob, env):
    E = pkg("engine")
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return E.Engine(blob, device=0, n_conv_slots=8192)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module", params=["scan_count", "count_pass"])
def eng(compiled, request):
    e = _engine(compiled.blob, {"PII_SCAN_COUNT": "0"} if request.param == "count_pass" else {})
    yield e
    e.close()


@pytest.fixture(scope="module")
def ref(compiled):
    """the count-pass engine every case is also compared with (its own context store: each case
    uses conversation slots no earlier case touched, in both engines)"""
    e = _engine(compiled.blob, {"PII_SCAN_COUNT": "0"})
    yield e
    e.close()


@pytest.fixture(scope="module")
def sim(compiled):
    from tablesim import TableSim
    return TableSim(compiled)


def _fill(n):
    return (FILL * (n // len(FILL) + 1))[:n]


def _sim_counts(sim, text):
    """(pairs, keyword events, events) of one row: pairs = sum over events of the accept set's pattern
    list length (what tools/pair_stats.py sums)"""
    pairs = kws = 0
    ev = sim.scan(text, True)
    for pos, sd, sk in ev:
        cd, ck = sim._classes(text, pos)
        a = int(sim.dacc[sd, cd])
        pairs += int(sim.d_off[a + 1]) - int(sim.d_off[a])
        kws += 1 if int(sim.kacc[sk, ck]) else 0
    return pairs, kws, len(ev)


def _run(e, rows):
    e.histogram_reset()
    res = e.scan_redact([t for _, _, t, _ in rows], [c for c, _, _, _ in rows], [r for _, r, _, _ in rows],
                        [s for _, _, _, s in rows])
    return res, e.histogram().copy(), e.queue_sizes(), e.stats()


def _spans(res, i):
    m = res.spans["utt"] == i
    return [(int(s["start"]), int(s["end"]), int(s["info_type"]), int(s["likelihood"])) for s in res.spans[m]]


def _check(eng, ref, rows, cfg, store=None):
    """one batch on both engines: bit-equal to each other, and to the oracle (rows: conv, role, text, ts)"""
    from oracle import pii_oracle as O
    got = _run(eng, rows)
    want = _run(ref, rows)
    res, hist, qs, st = got
    r2, h2, q2, s2 = want
    assert st["lane_bytes"] == LANE
    assert np.array_equal(res.out, r2.out)
    assert np.array_equal(res.out_offsets, r2.out_offsets)
    assert np.array_equal(res.spans, r2.spans)
    assert np.array_equal(res.ctx_info, r2.ctx_info)
    assert np.array_equal(hist, h2)
    assert qs == q2, (qs, q2)
    assert st == s2
    exp = O.process_rows(rows, cfg, store=store)
    groups = list(cfg.context_keywords.keys())
    ohist = np.zeros(len(hist), dtype=np.uint64)
    offs = [0]
    for i, ((red, fs, used, stored), row) in enumerate(zip(exp, rows)):
        assert res.text(i) == red, (i, row[2][:80], res.text(i)[:80], red[:80])
        assert _spans(res, i) == [(f.start, f.end, f.type_id, f.likelihood) for f in fs], (i, row[2][:80])
        g = int(res.ctx_info[i])
        assert (groups[g] if g >= 0 else None) == (stored if row[1] == O.ROLE_AGENT else used), (i, row[2][:80])
        for f in fs:
            ohist[f.type_id] += 1
        offs.append(offs[-1] + len(red))
    assert [int(x) for x in res.out_offsets] == offs
    assert np.array_equal(hist, ohist)
    return res, qs, st


_SLOT = [0]


def _slots(n):
    """n conversation slots no earlier case used (the context store persists in an engine)"""
    b = _SLOT[0]
    _SLOT[0] += n
    assert _SLOT[0] <= 8192
    return b


# ------------------------------------------------------------------ 1. keyword without a candidate
def test_keyword_without_candidate(eng, ref, oracle_cfg, sim):
    from oracle import pii_oracle as O
    A, C = O.ROLE_AGENT, O.ROLE_CUSTOMER
    for t in KW_ONLY:
        p, k, _ = _sim_counts(sim, t)
        assert p == 0 and k >= 1, (t, p, k)
    b = _slots(16)
    rows, ts = [], 1_000_000
    for k, (q, v) in enumerate(zip(KW_ONLY, VALUES)):
        rows += [(b + k, A, q, ts), (b + k, C, v, ts + 1)]
        ts += 2
    # an AGENT row alone in its lane: it starts on a lane boundary (a filler row pads up to it) and is
    # longer than the lane, so no other row starts there
    used = sum(len(t) for _, _, t, _ in rows)
    rows.append((b + 8, C, _fill(2 * LANE - used % LANE), ts))
    alone = _fill(LANE + 12 - len(KW_ONLY[3]) - 1) + b" " + KW_ONLY[3]
    p, k, _ = _sim_counts(sim, alone)
    assert p == 0 and k >= 1 and len(alone) == LANE + 12
    assert sum(len(t) for _, _, t, _ in rows) % LANE == 0
    i_alone = len(rows)
    rows += [(b + 9, A, alone, ts + 1), (b + 9, C, VALUES[3], ts + 2)]
    # ... and one that is the last row of the batch: its CUSTOMER row comes with the next call
    rows.append((b + 10, A, KW_ONLY[0], ts + 3))
    store = O.ContextStore()
    res, _, _ = _check(eng, ref, rows, oracle_cfg, store)
    for i, (_, role, _, _) in enumerate(rows):
        if role == A or (i > 0 and rows[i - 1][1] == A):
            assert int(res.ctx_info[i]) >= 0, (i, rows[i][2])          # the keyword group arrived
    assert int(res.ctx_info[i_alone]) >= 0 and int(res.ctx_info[-1]) >= 0
    res2, _, _ = _check(eng, ref, [(b + 10, C, VALUES[0], ts + 4)], oracle_cfg, store)
    assert int(res2.ctx_info[0]) >= 0


# ------------------------------------------------------------------ 2. lane-count edges
@functools.lru_cache(maxsize=None)
def _bank():
    return pkg("synth").build_bank(200, 200, seed=43)


def _rows_for_lanes(n_lanes, slot_base, seed):
    """short bank rows (AGENT / CUSTOMER alternating, two per conversation) filling n_lanes lanes: the
    batch is 128 n_lanes - 64 bytes, n_lanes lanes wherever the buffer's first 64-byte line starts"""
    from oracle import pii_oracle as O
    bank = _bank()
    na = int((bank.roles == 1).sum())
    r = random.Random(seed)
    total = LANE * n_lanes - 64
    rows, used, k = [], 0, 0
    while True:
        t = bank.texts[r.randrange(na) if k % 2 == 0 else na + r.randrange(len(bank.texts) - na)]
        if used + len(t) > total:
            break
        rows.append((slot_base + k // 2, O.ROLE_AGENT if k % 2 == 0 else O.ROLE_CUSTOMER, t, 1_000_000 + k))
        used += len(t)
        k += 1
    rows.append((slot_base + k // 2 + 1, O.ROLE_CUSTOMER, _fill(total - used), 1_000_000 + k))
    return rows


def test_one_row(eng, ref, oracle_cfg):
    from oracle import pii_oracle as O
    b = _slots(1)
    _, qs, st = _check(eng, ref, [(b, O.ROLE_CUSTOMER, b"my card is 4111 1111 1111 1111, thanks", 5)], oracle_cfg)
    assert st["lanes"] == 1 and qs[0] > 0


@pytest.mark.parametrize("n_lanes", [63, 64, 65, 255, 256, 257])
def test_lane_count_edges(eng, ref, oracle_cfg, n_lanes):
    """wavefront (64) and workgroup (256) boundaries of k_pairs_flat"""
    rows = _rows_for_lanes(n_lanes, _slots(400), seed=n_lanes)
    _, qs, st = _check(eng, ref, rows, oracle_cfg)
    assert st["lanes"] == n_lanes and qs[0] > 0


def test_empty_rows_and_lanes_then_smaller_batch(eng, ref, oracle_cfg, sim):
    """empty rows, lanes without any event (their pair count is written as 0), and a smaller batch
    after a larger one on the same engine (no count of the larger call may survive)"""
    from oracle import pii_oracle as O
    C = O.ROLE_CUSTOMER
    quiet = b"okay okay okay then " * 10                      # 200 bytes, no event: whole quiet lanes
    assert _sim_counts(sim, quiet)[2] == 0
    big = _rows_for_lanes(257, _slots(400), seed=7)
    _check(eng, ref, big, oracle_cfg)
    b = _slots(64)
    texts = []
    for k in range(12):
        texts += [b"", quiet, quiet]
        if k % 4 == 1:
            texts.append(b"reach me at jane.doe@example.com or 10.1.2.3")
        texts.append(b"")
    rows = [(b + i, C, t, 10 + i) for i, t in enumerate(texts)]        # (one conversation per row)
    assert len(rows) < 62
    _, qs, st = _check(eng, ref, rows, oracle_cfg)
    assert 30 < st["lanes"] < 257 and qs[0] > 0
    # the same engine again, a batch with no pair at all where the last one had some
    _, qs, _ = _check(eng, ref, [(b + 63, C, quiet, 99), (b + 62, C, b"", 99)], oracle_cfg)
    assert qs[0] == 0


# ------------------------------------------------------------------ 3. dense events
def test_dense_events(eng, ref, oracle_cfg):
    """more than 64 events in one wavefront's lanes (the flattened 64-event chunks of k_pairs_flat),
    lanes not a multiple of 64"""
    from oracle import pii_oracle as O
    r = random.Random(41)
    b = _slots(64)
    rows = []
    for k in range(20):
        n = r.randrange(20, 120)
        items = [f"u{r.randrange(10 ** 6)}@x{r.randrange(9)}.io" if r.random() < 0.7 else
                 f"10.{r.randrange(256)}.{r.randrange(256)}.{r.randrange(256)}" for _ in range(n)]
        rows.append((b + k, O.ROLE_CUSTOMER, " ".join(items).encode(), 100 + k))
        rows.append((b + 20 + k, O.ROLE_CUSTOMER, b"ok thanks" if k % 3 else b"", 100 + k))
    total = sum(len(t) for _, _, t, _ in rows)
    if ((total + LANE - 1) // LANE) % 64 in (0, 63):           # (keep clear of a multiple of 64 for any alignment)
        rows.append((b + 60, O.ROLE_CUSTOMER, _fill(3 * LANE), 200))
    _, qs, st = _check(eng, ref, rows, oracle_cfg)
    assert st["lanes"] % 64 != 0
    assert qs[1] > 4 * st["lanes"]                             # events: several per lane on average


# ------------------------------------------------------------------ 4. re-scanned cut lanes
def test_rescanned_cut_lanes(eng, ref, oracle_cfg):
    """a 300-byte unbroken token ending in an address straddles the cuts of a >= 4-lane row: the halo
    (128 bytes) cannot reproduce the state at a cut further than that from the '@', k_scan_fix
    re-scans the lane and its events -- and so its pair count -- change"""
    from oracle import pii_oracle as O
    r = random.Random(5)
    b = _slots(16)
    rows, long_rows = [], []
    for k, shift in enumerate((0, 37, 90, 121)):
        run = "".join(r.choice("abcdefghijklmnopqrstuvwxyz0123456789.") for _ in range(298))
        run = "a" + run.replace("..", ".x") + "b"
        assert len(run) == 300
        text = (_fill(shift) + b"card 4111 1111 1111 1111 and ssn 536-22-8726 then " + run.encode() +
                b"@example.com, after that 10.20.30.40 and (415) 555-0132 " + _fill(120))
        assert len(text) >= 4 * LANE
        rows.append((b + 2 * k, O.ROLE_CUSTOMER, b"hello there", 50 + k))
        long_rows.append(len(rows))
        rows.append((b + 2 * k + 1, O.ROLE_CUSTOMER, text, 50 + k))
    res, qs, _ = _check(eng, ref, rows, oracle_cfg)               # (the pair totals are compared in _check)
    assert qs[0] > 0
    for i in long_rows:
        sp = _spans(res, i)
        assert any(e - s >= 300 for s, e, _, _ in sp), (i, sp)   # the address with its whole local part
        off = sum(len(t) for _, _, t, _ in rows[:i])
        assert len({(off + s) // LANE for s, _, _, _ in sp}) >= 2, (i, sp)


# ------------------------------------------------------------------ 5. CPU reference for the count
@functools.lru_cache(maxsize=None)
def _corpus_1500():
    synth = pkg("synth")
    bank = synth.build_bank(256, 256, seed=synth.SEED)
    meta = synth.corpus_meta(15, 100, bank, seed=synth.SEED)
    data = synth.gather_bytes(meta, bank)
    o = meta.offsets
    return meta, [data[int(o[i]):int(o[i + 1])].tobytes() for i in range(meta.n)]


@pytest.fixture(scope="module")
def sim_pairs(sim):
    _, texts = _corpus_1500()
    return sum(_sim_counts(sim, t)[0] for t in texts)


def test_pair_count_vs_tablesim(eng, sim_pairs):
    meta, texts = _corpus_1500()
    b = _slots(16)
    eng.scan_redact(texts, (meta.conv_slot + b).tolist(), meta.role.tolist(), meta.ts_us.tolist())
    assert eng.stats()["lane_bytes"] == LANE
    assert eng.queue_sizes()[0] == sim_pairs


# ------------------------------------------------------------------ 6. one window re-scan step
def test_window_rescan(compiled, oracle_cfg):
    from oracle import pii_oracle as O
    synth = pkg("synth")
    bank = _bank()
    corp = synth.make_corpus(60, 5, bank, seed=11)
    rows = [(int(corp.conv_slot[i]), int(corp.role[i]),
             corp.data[int(corp.offsets[i]):int(corp.offsets[i + 1])].tobytes(), int(corp.ts_us[i]))
            for i in range(corp.n)]
    # an AGENT row with nothing but a keyword, then the value, inside one conversation's window
    rows += [(100, O.ROLE_AGENT, KW_ONLY[1], 1), (100, O.ROLE_CUSTOMER, VALUES[1], 2),
             (101, O.ROLE_AGENT, KW_ONLY[0], 1)]
    outs = []
    for env in ({}, {"PII_SCAN_COUNT": "0"}):
        e = _engine(compiled.blob, env)
        try:
            e.window_enable(5, 8192, full=False)
            assert e.window_mode() == "incremental"
            store, hist = O.ContextStore(), {}
            groups = list(oracle_cfg.context_keywords.keys())
            calls = (rows, [(101, O.ROLE_CUSTOMER, VALUES[0], 2)])
            for call in calls:
                res = e.rescan_window([t for _, _, t, _ in call], [c for c, _, _, _ in call],
                                      [r for _, r, _, _ in call], [s for _, _, _, s in call])
                exp = O.process_window_rows(call, oracle_cfg, n=5, store=store, history=hist)
                for i, ((red, fs, et), row) in enumerate(zip(exp, call)):
                    assert res.text(i) == red, (i, row, res.text(i), red)
                    assert _spans(res, i) == [(f.start, f.end, f.type_id, f.likelihood) for f in fs], (i, row)
                    g = int(res.ctx_info[i])
                    assert (groups[g] if g >= 0 else None) == et, (i, row)
                outs.append((res.out.tobytes(), res.out_offsets.tobytes(), res.spans.copy(), res.ctx_info.tobytes(),
                             e.queue_sizes()))
        finally:
            e.close()
    half = len(outs) // 2
    for a, c in zip(outs[:half], outs[half:]):
        assert a[0] == c[0] and a[1] == c[1] and np.array_equal(a[2], c[2]) and a[3] == c[3] and a[4] == c[4]
