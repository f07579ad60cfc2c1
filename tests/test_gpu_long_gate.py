"""The long-row gate: a scan-and-redact call launches the long-row kernels (k_fill_long, k_scan_fix,
k_sel_dirty, k_sel_fix, k_rowlen) only while the engine expects rows that are cut into several lanes.
A cut row in a call launched without them fails that call on the device (nothing is committed) and
pii_sync runs it again with them; after LONG_IDLE_CALLS calls without a cut row the gate closes again.
PII_LONG_GATE=0 launches them always.

Nothing a caller sees may depend on the gate: every batch runs on a gated engine and on one created
under PII_LONG_GATE=0, which must agree bit for bit (output bytes, out_offsets, spans, per-row
context, histogram), and both with the oracle.  Batches this small get 128-byte lanes (cuts at every
multiple of 128 bytes of the batch: the staging buffers are 64-byte aligned), so a row longer than
256 bytes that crosses a slice boundary is a cut row: the smallest shapes at which this can go wrong.
"""
import os
import random

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

LANE = 128
LONG_IDLE_CALLS = 8          # (pii_engine.hip)
FILL = b"please note that the shipment will arrive on monday morning before noon at the usual place "
N_SLOTS = 8192


def _engine(blob, env):
    E = pkg("engine")
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return E.Engine(blob, device=0, n_conv_slots=N_SLOTS)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ref(compiled):
    """the engine whose gate is off (each case uses conversation slots no earlier case touched)"""
    e = _engine(compiled.blob, {"PII_LONG_GATE": "0"})
    yield e
    e.close()


@pytest.fixture()
def eng(compiled):
    """a fresh gated engine: its gate is closed"""
    e = _engine(compiled.blob, {})
    yield e
    e.close()


_SLOT = [0]


def _slots(n):
    b = _SLOT[0]
    _SLOT[0] += n
    assert _SLOT[0] <= N_SLOTS
    return b


def _fill(n):
    return (FILL * (n // len(FILL) + 1))[:n]


def _dense(r, n):
    """exactly n bytes of PII values a space apart (k_sel_fix has work wherever a cut falls)"""
    out = b""
    while len(out) < n:
        k = r.randrange(5)
        item = (f"u{r.randrange(10 ** 5)}@x{r.randrange(9)}.io" if k == 0 else
                f"10.{r.randrange(256)}.{r.randrange(256)}.{r.randrange(256)}" if k == 1 else
                "536-22-8726" if k == 2 else "4111 1111 1111 1111" if k == 3 else "(415) 555-0132")
        out += item.encode() + b" "
    return out[:n]


def _sparse(r, n):
    """exactly n bytes: a PII value after every 60 bytes of filler (few enough candidate pairs that a
    batch of such rows stays inside the pair queue's first sizing: no queue re-run in the counts)"""
    out = b""
    while len(out) < n:
        out += _fill(60) + _dense(r, 20).rsplit(b" ", 1)[0] + b" "
    return out[:n]


def _short_rows(r, n, slot_base, ts0=1_000_000):
    """n rows of at most 200 bytes, AGENT question / CUSTOMER answer pairs among plain ones"""
    from oracle import pii_oracle as O
    rows = []
    for k in range(n):
        c = r.randrange(4)
        if c == 0:
            rows.append((slot_base + k, O.ROLE_AGENT, b"could you read me the card number please", ts0 + k))
        elif c == 1:
            rows.append((slot_base + k, O.ROLE_CUSTOMER, b"reach me at jane.doe@example.com or (415) 555-0132", ts0 + k))
        elif c == 2:
            rows.append((slot_base + k, O.ROLE_CUSTOMER, _fill(r.randrange(0, 200)), ts0 + k))
        else:
            rows.append((slot_base + k, O.ROLE_CUSTOMER, _dense(r, r.randrange(20, 200)), ts0 + k))
    assert all(len(t) <= 200 for _, _, t, _ in rows)
    return rows


def _pad_to(rows, phase, slot, ts=5):
    """a filler row after which the batch is `phase` bytes past a slice boundary"""
    from oracle import pii_oracle as O
    used = sum(len(t) for _, _, t, _ in rows)
    rows.append((slot, O.ROLE_CUSTOMER, _fill((phase - used) % LANE), ts))


def _long_row(start, r):
    """~700 bytes starting `start` bytes into the batch: a card number over the first cut, a hotword
    that ends on the second cut with its value behind it, an address whose 300-byte local part lies
    over two cuts (further from the '@' than the scan's 128-byte halo), then dense PII"""
    t = b""

    def upto(pos):                      # filler up to batch position pos
        nonlocal t
        assert start + len(t) <= pos
        t += _fill(pos - start - len(t))

    cut = (start // LANE + 1) * LANE
    upto(cut - 8)
    t += b" 4111 1111 1111 1111 "
    hot = b" my social security number is"
    upto(cut + LANE - len(hot))
    t += hot + b" 536-22-8726 and then "
    run = "".join(r.choice("abcdefghijklmnopqrstuvwxyz0123456789") for _ in range(300))
    t += run.encode() + b"@example.com, "
    t += _dense(r, 160)
    assert 600 <= len(t) <= 800
    return t


class _Dev:
    """a batch through pii_scan_redact_device_ex: enqueue (no device-to-host read), then sync"""

    def __init__(self, e, rows):
        import torch
        E = pkg("engine")
        dev = torch.device("cuda", 0)
        data, offs = E.pack([t for _, _, t, _ in rows])
        n, nb = len(rows), int(offs[-1])
        out_cap, span_cap = nb + 48 * n + 64, nb // 3 + n + 16
        d_text = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).to(dev)
        d_offs = torch.from_numpy(offs.view(np.int64).copy()).to(dev)
        d_slot = torch.tensor([c for c, _, _, _ in rows], dtype=torch.int32, device=dev)
        d_role = torch.tensor([x for _, x, _, _ in rows], dtype=torch.uint8, device=dev)
        d_ts = torch.tensor([s for _, _, _, s in rows], dtype=torch.int64, device=dev)
        d_out = torch.zeros(out_cap + 16, dtype=torch.uint8, device=dev)
        d_oo = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_sp = torch.zeros(span_cap * 16, dtype=torch.uint8, device=dev)
        d_ctx = torch.zeros(n, dtype=torch.int16, device=dev)
        e.scan_redact_device_ex(d_text.data_ptr(), d_offs.data_ptr(), n, 0, nb, d_slot.data_ptr(), d_role.data_ptr(),
                                d_ts.data_ptr(), d_out.data_ptr(), out_cap, d_oo.data_ptr(), d_sp.data_ptr(), span_cap,
                                d_ctx.data_ptr())
        ob, ns, fl = e.sync()
        assert fl == 0
        self.out_offsets = d_oo.cpu().numpy().view(np.uint64)
        assert ob == int(self.out_offsets[-1])
        self.out = d_out.cpu().numpy()[:ob]
        self.spans = d_sp.cpu().numpy()[:ns * 16].view(E.SPAN_DTYPE)
        self.ctx_info = d_ctx.cpu().numpy()

    def text(self, i):
        return self.out[int(self.out_offsets[i]):int(self.out_offsets[i + 1])].tobytes()


def _run(e, rows, device):
    e.histogram_reset()
    if device:
        res = _Dev(e, rows)
    else:
        res = e.scan_redact([t for _, _, t, _ in rows], [c for c, _, _, _ in rows], [x for _, x, _, _ in rows],
                            [s for _, _, _, s in rows])
    return res, e.histogram().copy(), e.stats(gate=True)


def _spans(res, i):
    m = res.spans["utt"] == i
    return [(int(s["start"]), int(s["end"]), int(s["info_type"]), int(s["likelihood"])) for s in res.spans[m]]


def _check(eng, ref, rows, cfg, store=None, device=False):
    """one batch on both engines: bit-equal to each other and to the oracle; returns the gated engine's
    result and its stats (rows: conv, role, text, ts)"""
    from oracle import pii_oracle as O
    res, hist, st = _run(eng, rows, device)
    r2, h2, s2 = _run(ref, rows, device)
    assert st["lane_bytes"] == LANE and s2["lane_bytes"] == LANE
    assert np.array_equal(res.out, r2.out)
    assert np.array_equal(res.out_offsets, r2.out_offsets)
    assert np.array_equal(res.spans, r2.spans)
    assert np.array_equal(res.ctx_info, r2.ctx_info)
    assert np.array_equal(hist, h2)
    assert {k: st[k] for k in ("pairs", "events", "lanes", "spans", "cut_rows")} == \
           {k: s2[k] for k in ("pairs", "events", "lanes", "spans", "cut_rows")}
    assert s2["long_kernels_launched"] == 1 and s2["reruns"] == 0       # gate off: always, never
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
            ohist[f.type_id] += 1           # each finding once, also after a re-run
        offs.append(offs[-1] + len(red))
    assert [int(x) for x in res.out_offsets] == offs
    assert np.array_equal(hist, ohist)
    return res, st


def _long_batch(r, b, ts0):
    """short rows around one ~700-byte row, and an AGENT row whose context the next call reads"""
    from oracle import pii_oracle as O
    rows = _short_rows(r, 6, b, ts0)
    _pad_to(rows, 40, b + 6, ts0 + 6)
    i_long = len(rows)
    rows.append((b + 7, O.ROLE_CUSTOMER, _long_row(sum(len(t) for _, _, t, _ in rows), r), ts0 + 7))
    rows += _short_rows(r, 4, b + 8, ts0 + 8)
    rows.append((b + 12, O.ROLE_AGENT, b"what is your social security number", ts0 + 12))
    return rows, i_long


# ------------------------------------------------ 1-5. the gate over a sequence of calls, both entry points
@pytest.mark.parametrize("device", [False, True], ids=["host", "device_ex"])
def test_gate_sequence(eng, ref, oracle_cfg, device):
    from oracle import pii_oracle as O
    r = random.Random(11 + device)
    store = O.ContextStore()
    b = _slots(400)
    ts = 1_000_000
    # 1. a fresh engine, short rows only
    _, st = _check(eng, ref, _short_rows(r, 40, b, ts), oracle_cfg, store, device)
    assert (st["cut_rows"], st["long_kernels_launched"], st["reruns"]) == (0, 0, 0)
    # 2. a long row arrives: run without the long-row kernels, refused, run again with them
    rows, i_long = _long_batch(r, b + 40, ts + 100)
    res, st = _check(eng, ref, rows, oracle_cfg, store, device)
    assert st["cut_rows"] >= 1 and (st["long_kernels_launched"], st["reruns"]) == (1, 1)
    sp = _spans(res, i_long)
    lo = sum(len(t) for _, _, t, _ in rows[:i_long])
    assert sum(1 for s, e, _, _ in sp if (lo + s) // LANE != (lo + e - 1) // LANE) >= 2, sp     # PII over cuts
    assert any(e - s >= 300 for s, e, _, _ in sp), sp                  # the address with its whole local part
    # the AGENT row's context was committed once, by the re-run: the next call's customer row reads it
    nxt = [(b + 40 + 12, O.ROLE_CUSTOMER, b"sure it is 536-22-8726", ts + 120)]
    rows3, _ = _long_batch(r, b + 60, ts + 200)
    res, st = _check(eng, ref, nxt + rows3, oracle_cfg, store, device)
    assert int(res.ctx_info[0]) >= 0
    # 3. ... which has a long row again: launched, no re-run
    assert st["cut_rows"] >= 1 and (st["long_kernels_launched"], st["reruns"]) == (1, 0)
    # 4. LONG_IDLE_CALLS batches without one: launched for each of them, then not again
    for k in range(LONG_IDLE_CALLS):
        _, st = _check(eng, ref, _short_rows(r, 9, b + 100 + 10 * k, ts + 300 + 10 * k), oracle_cfg, store, device)
        assert (st["cut_rows"], st["long_kernels_launched"], st["reruns"]) == (0, 1, 0), k
    _, st = _check(eng, ref, _short_rows(r, 9, b + 200, ts + 400), oracle_cfg, store, device)
    assert (st["cut_rows"], st["long_kernels_launched"], st["reruns"]) == (0, 0, 0)
    rows, _ = _long_batch(r, b + 220, ts + 500)
    _, st = _check(eng, ref, rows, oracle_cfg, store, device)
    assert st["cut_rows"] >= 1 and (st["long_kernels_launched"], st["reruns"]) == (1, 1)


# ------------------------------------------------ 6. cut rows at the edges of the slice list, gate closed
def _edge_rows(case, r, b):
    """(rows, cut rows): the c_lo / c_hi edges of the serial first_utt fill"""
    from oracle import pii_oracle as O
    C = O.ROLE_CUSTOMER
    short = lambda k: (b + k, C, b"reach me at jane.doe@example.com please", 10 + k)      # noqa: E731
    if case == "first_row":
        return [(b, C, _dense(r, 400), 9), short(1), short(2)], 1
    if case == "last_row":
        return [short(0), short(1), (b + 2, C, _dense(r, 400), 12)], 1
    if case == "adjacent":
        return [short(0), (b + 1, C, _dense(r, 300), 11), (b + 2, C, _dense(r, 470), 12), short(3)], 2
    if case == "ends_on_boundary":
        rows = [short(0)]
        _pad_to(rows, 40, b + 1)
        rows.append((b + 2, C, _dense(r, 3 * LANE + 88), 12))
        assert sum(len(t) for _, _, t, _ in rows) % LANE == 0
        return rows + [short(3)], 1
    if case == "ends_on_boundary_last":
        rows = [short(0)]
        _pad_to(rows, 40, b + 1)
        rows.append((b + 2, C, _dense(r, 3 * LANE + 88), 12))
        return rows, 1
    raise AssertionError(case)


@pytest.mark.parametrize("case", ["first_row", "last_row", "adjacent", "ends_on_boundary", "ends_on_boundary_last"])
def test_cut_rows_at_the_edges(eng, ref, oracle_cfg, case):
    rows, n_cut = _edge_rows(case, random.Random(len(case)), _slots(8))
    _, st = _check(eng, ref, rows, oracle_cfg)
    assert (st["cut_rows"], st["long_kernels_launched"], st["reruns"]) == (n_cut, 1, 1)


# ------------------------------------------------ 7. several cut rows in one closed-gate call
def test_many_cut_rows_closed_gate(eng, ref, oracle_cfg):
    """cut rows in one wavefront's ballot of k_chunk_index (4 rows per thread) and in several
    wavefronts and workgroups: the listing and the serial fill together"""
    from oracle import pii_oracle as O
    r = random.Random(3)
    b = _slots(1400)
    rows, n_cut = [], 0
    for k in range(1300):
        if k % 97 in (5, 6, 40) or k == 1299:
            rows.append((b + k, O.ROLE_CUSTOMER, _sparse(r, r.randrange(2 * LANE + 130, 5 * LANE)), 100 + k))
            n_cut += 1                  # (longer than two lanes + a lane: cut wherever it starts)
        else:
            rows.append((b + k, O.ROLE_CUSTOMER, _fill(r.randrange(0, 30)) if k % 3 else b"call (415) 555-0132", 100 + k))
    assert n_cut > 30 and len(rows) > 1024
    _, st = _check(eng, ref, rows, oracle_cfg)
    assert (st["cut_rows"], st["long_kernels_launched"], st["reruns"]) == (n_cut, 1, 1)


# ------------------------------------------------ 8. the re-run keeps the call's external candidates
def test_rerun_carries_external_candidates(eng, oracle_cfg):
    """a closed-gate call with a cut row and a row with two external spans: pii_sync's re-run is the
    same call, external candidates included (output, spans and histogram as the oracle's with them)"""
    from oracle import pii_oracle as O
    P = oracle_cfg.type_id["PERSON_NAME"]
    rows, n_cut = _edge_rows("first_row", random.Random(8), _slots(8))
    assert len(rows) == 3 and all(x == O.ROLE_CUSTOMER for _, x, _, _ in rows)
    assert rows[1][2] == b"reach me at jane.doe@example.com please"
    ext = [[], [(0, 5, P, 4), (33, 39, P, 5)], []]                     # "reach", "please"
    eng.histogram_reset()
    res = eng.scan_redact([t for _, _, t, _ in rows], [c for c, _, _, _ in rows], [x for _, x, _, _ in rows],
                          [s for _, _, _, s in rows], ext=ext)
    st = eng.stats(gate=True)
    assert st["lane_bytes"] == LANE
    assert (st["cut_rows"], st["long_kernels_launched"], st["reruns"]) == (n_cut, 1, 1)
    hist = eng.histogram()
    ohist = np.zeros(len(hist), dtype=np.uint64)
    exp = O.process_rows(rows, oracle_cfg, extra=ext)
    for i, (red, fs, _, _) in enumerate(exp):
        assert res.text(i) == red, (i, res.text(i)[:80], red[:80])
        assert _spans(res, i) == [(f.start, f.end, f.type_id, f.likelihood) for f in fs], i
        for f in fs:
            ohist[f.type_id] += 1
    assert [(f.start, f.end) for f in exp[1][1] if f.type_id == P] == [(0, 5), (33, 39)]
    assert np.array_equal(hist, ohist)
