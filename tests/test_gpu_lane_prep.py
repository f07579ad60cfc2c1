"""Lane preparation: k_lane_place writes each lane's utterance-start words at the slot it hands the
lane (the default), against the path that hands the slots to a separate k_lane_bits launch through
lane_pos (PII_LANE_PREP=0).

Nothing a caller sees may depend on the knob: every batch runs on one engine per setting, which must
agree bit for bit (output bytes, out_offsets, spans, per-row context, histogram, work sizes and the
long-row gate's record), and with the oracle.  Batches this small get 128-byte lanes (MIN_LANE_SHIFT)
and rows longer than 256 bytes are cut, so the shapes below are the smallest at which the lane
records, the staged row offsets (WROWS_CAP = 2048 rows per wavefront) and the slices' edges can go
wrong.
"""
import os
import random

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

LANE = 128
LONG_IDLE_CALLS = 8          # (pii_engine.hip)
LANE_SORT_CHUNK = 1024       # lanes per k_lane_count / k_lane_place workgroup
LANE_NB = 128                # length buckets of 32 bytes
FILL = b"please note that the shipment will arrive on monday morning before noon at the usual place "
N_SLOTS = 1 << 16
PREPS = ("1", "0")         # the last one is the reference
STAT_KEYS = ("pairs", "events", "lanes", "lane_bytes", "spans", "cut_rows", "long_kernels_launched", "reruns")


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


def _engines(blob):
    return [_engine(blob, {"PII_LANE_PREP": p}) for p in PREPS]


@pytest.fixture(scope="module")
def engs(compiled):
    """one engine per PII_LANE_PREP setting; their long-row gates stay closed (no case here has a cut row)"""
    es = _engines(compiled.blob)
    yield es
    for e in es:
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
    """exactly n bytes of PII values a space apart"""
    out = b""
    while len(out) < n:
        k = r.randrange(5)
        item = (f"u{r.randrange(10 ** 5)}@x{r.randrange(9)}.io" if k == 0 else
                f"10.{r.randrange(256)}.{r.randrange(256)}.{r.randrange(256)}" if k == 1 else
                "536-22-8726" if k == 2 else "4111 1111 1111 1111" if k == 3 else "(415) 555-0132")
        out += item.encode() + b" "
    return out[:n]


def _sparse(r, n):
    """exactly n bytes: a PII value after every 60 bytes of filler"""
    out = b""
    while len(out) < n:
        out += _fill(60) + _dense(r, 20).rsplit(b" ", 1)[0] + b" "
    return out[:n]


class _Rows:
    """a batch under construction: rows (conv, role, text, ts), one conversation per row"""

    def __init__(self, r, slot_base):
        self.r, self.b, self.rows = r, slot_base, []

    @property
    def used(self):
        return sum(len(t) for _, _, t, _ in self.rows)

    def add(self, text, agent=False):
        from oracle import pii_oracle as O
        k = len(self.rows)
        self.rows.append((self.b + k, O.ROLE_AGENT if agent else O.ROLE_CUSTOMER, text, 1000 + k))

    def short(self, n, hi=200):
        for _ in range(n):
            c = self.r.randrange(4)
            if c == 0:
                self.add(b"could you read me the card number please", agent=True)
            elif c == 1:
                self.add(b"reach me at jane.doe@example.com or (415) 555-0132")
            elif c == 2:
                self.add(_fill(self.r.randrange(0, hi)))
            else:
                self.add(_dense(self.r, self.r.randrange(20, hi)))

    def pad_to(self, phase):
        """a filler row after which the batch is `phase` bytes past a slice boundary"""
        self.add(_fill((phase - self.used) % LANE))


def _lane_lengths(rows, r0=0):
    """the scan lanes' byte lengths when no row is cut: from the first row start in a slice to the
    first one in a later slice (0 for a slice in which no row starts)"""
    total = sum(len(t) for _, _, t, _ in rows)
    n_lanes = (total + r0 + LANE - 1) // LANE
    first = [None] * (n_lanes + 1)
    pos = 0
    for _, _, t, _ in rows:
        c = (pos + r0) // LANE
        if c < n_lanes and first[c] is None:
            first[c] = pos
        pos += len(t)
    nxt, lens = total, [0] * n_lanes
    for c in range(n_lanes - 1, -1, -1):
        if first[c] is not None:
            lens[c] = nxt - first[c]
            nxt = first[c]
    return lens


class _Dev:
    """a batch through pii_scan_redact_device_ex, its text `shift` bytes into a device tensor"""

    def __init__(self, e, rows, shift):
        import torch
        E = pkg("engine")
        dev = torch.device("cuda", 0)
        data, offs = E.pack([t for _, _, t, _ in rows])
        n, nb = len(rows), int(offs[-1])
        out_cap, span_cap = nb + 48 * n + 64, nb // 3 + n + 16
        buf = torch.zeros(nb + shift + 80, dtype=torch.uint8, device=dev)
        assert buf.data_ptr() % 64 == 0
        buf[shift:shift + nb] = torch.from_numpy(data.copy()).to(dev)
        d_text = buf[shift:]
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


def _run(e, rows, shift):
    e.histogram_reset()
    if shift is None:
        res = e.scan_redact([t for _, _, t, _ in rows], [c for c, _, _, _ in rows], [x for _, x, _, _ in rows],
                            [s for _, _, _, s in rows])
    else:
        res = _Dev(e, rows, shift)
    st = e.stats(gate=True)
    return res, e.histogram().copy(), {k: st[k] for k in STAT_KEYS}


def _spans(res, i):
    m = res.spans["utt"] == i
    return [(int(s["start"]), int(s["end"]), int(s["info_type"]), int(s["likelihood"])) for s in res.spans[m]]


def _same(a, b):
    (ra, ha, sa), (rb, hb, sb) = a, b
    assert np.array_equal(ra.out, rb.out)
    assert np.array_equal(ra.out_offsets, rb.out_offsets)
    assert np.array_equal(ra.spans, rb.spans)
    assert np.array_equal(ra.ctx_info, rb.ctx_info)
    assert np.array_equal(ha, hb)
    assert sa == sb


def _check(engs, rows, cfg, store=None, shift=None):
    """one batch on every engine: bit-equal to the reference path's result and to the oracle; returns
    the default engine's result and stats"""
    from oracle import pii_oracle as O
    got = [_run(e, rows, shift) for e in engs]
    for g in got[:-1]:
        _same(g, got[-1])
    res, hist, st = got[0]
    assert st["lane_bytes"] == LANE or not rows
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
    return res, st


def _closed(st):
    """no cut row, and the long-row kernels were not launched (a re-run with a larger pair queue,
    which a batch dense with PII values gets, is no concern of the gate)"""
    return (st["cut_rows"], st["long_kernels_launched"]) == (0, 0)


# ------------------------------------------------ row counts around k_chunk_index's four rows per thread
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 9])
def test_row_counts(engs, oracle_cfg, n):
    b = _Rows(random.Random(100 + n), _slots(16))
    b.short(n)
    _, st = _check(engs, b.rows, oracle_cfg)
    assert _closed(st)
    if n:
        _check(engs, b.rows, oracle_cfg, store=None, shift=0)


# ------------------------------------------------ slice boundaries
def _boundary_rows(r, slot_base):
    """rows that start just before, exactly on and after slice boundaries, with empty rows at each of
    those places, a 1-byte row that ends on a boundary, and a batch that ends on one with empty rows"""
    b = _Rows(r, slot_base)
    b.add(_dense(r, 100))
    b.add(b"")
    b.add(_fill(27))
    assert b.used == LANE - 1
    b.add(b"")                            # empty row one byte before the boundary
    b.add(b"x")                           # ends on it
    assert b.used == LANE
    b.add(b"")                            # empty rows on the boundary
    b.add(b"")
    b.add(b"call (415) 555-0132 tomorrow")          # a row starting exactly on it
    b.add(b"")                            # and one after it
    b.short(3)
    b.pad_to(0)
    b.add(b"what is your social security number", agent=True)      # on a boundary again
    b.add(b"")
    b.pad_to(LANE - 1)
    b.add(b"536-22-8726")                 # starts on the last byte of a slice
    b.pad_to(0)
    for _ in range(3):
        b.add(b"")                        # the batch ends on a boundary, with empty rows on it
    assert b.used % LANE == 0
    return b.rows


def test_rows_on_slice_boundaries(engs, oracle_cfg):
    rows = _boundary_rows(random.Random(1), _slots(64))
    _, st = _check(engs, rows, oracle_cfg)
    assert _closed(st)


@pytest.mark.parametrize("kind", ["empty", "one_byte"])
def test_more_rows_than_a_wavefront_stages(engs, oracle_cfg, kind):
    """more than WROWS_CAP = 2048 rows start in one wavefront's 64 lanes: the staged offsets are not
    used, every offset comes from global memory"""
    r = random.Random(7)
    b = _Rows(r, _slots(4096))
    b.short(5)
    for k in range(2600):
        b.add(b"" if kind == "empty" else b"7" if k % 5 else b" ")
    b.short(12)
    assert b.used < 64 * LANE                 # all in the first wavefront's lanes
    _, st = _check(engs, b.rows, oracle_cfg)
    assert _closed(st)


def test_uncut_row_over_two_boundaries(engs, oracle_cfg):
    """a row of exactly long_min = 256 bytes that two boundaries cross is not cut: the lane between
    them holds no row start (lo == hi)"""
    r = random.Random(9)
    b = _Rows(r, _slots(64))
    b.short(4)
    b.pad_to(100)
    at = b.used
    b.add(_dense(r, 2 * LANE))
    b.short(3)
    lens = _lane_lengths(b.rows)
    assert lens[at // LANE + 1] == 0 and lens[at // LANE] > 0 and lens[at // LANE + 2] > 0
    _, st = _check(engs, b.rows, oracle_cfg)
    assert _closed(st)


def test_last_lane_without_a_row_start(engs, oracle_cfg):
    r = random.Random(10)
    b = _Rows(r, _slots(64))
    b.short(6)
    b.pad_to(90)
    b.add(_dense(r, 150))                     # ends 112 bytes into the next slice, the batch's last
    lens = _lane_lengths(b.rows)
    assert lens[-1] == 0 and lens[-2] > 150
    _, st = _check(engs, b.rows, oracle_cfg)
    assert _closed(st)


@pytest.mark.parametrize("shift", [1, 15, 17, 63])
def test_misaligned_text_base(engs, oracle_cfg, shift):
    """the text begins `shift` bytes past a 64-byte boundary (r0 = shift): slices are cut in the address
    space, so every boundary of the batch moves"""
    r = random.Random(20 + shift)
    rows = _boundary_rows(r, _slots(64))
    b = _Rows(r, _slots(256))
    b.short(40)
    b.pad_to(LANE - shift)                    # a row starting exactly on an address boundary
    b.add(b"reach me at jane.doe@example.com please")
    b.add(b"")
    b.short(30)
    _, st = _check(engs, rows + b.rows, oracle_cfg, shift=shift)
    assert _closed(st)


def test_several_sort_workgroups(engs, oracle_cfg):
    """a few thousand lanes: several LANE_SORT_CHUNK workgroups count, place and write words; lane
    lengths from 0 to over 300 bytes (every bucket a batch of 128-byte lanes without cut rows reaches)"""
    r = random.Random(30)
    b = _Rows(r, _slots(4096))
    while b.used < 2 * LANE_SORT_CHUNK * LANE + 5000:
        b.short(50, hi=257)
        b.add(b"")
    lens = _lane_lengths(b.rows)
    assert len(lens) > 2 * LANE_SORT_CHUNK and len(b.rows) < 4096
    assert len({n >> 5 for n in lens}) >= 10 and 0 in lens
    _, st = _check(engs, b.rows, oracle_cfg)
    assert _closed(st) and st["lanes"] == len(lens)


# ------------------------------------------------ a cut row: the gate opens, stays open, closes again
def _long_row(r, start):
    """~700 bytes starting `start` bytes into the batch, a card number over its first cut"""
    cut = (start // LANE + 1) * LANE
    t = _fill(cut - 8 - start) + b" 4111 1111 1111 1111 " + _sparse(r, 4 * LANE + 60)
    return t


def _long_batch(r, slot_base):
    b = _Rows(r, slot_base)
    b.short(6)
    b.pad_to(40)
    b.add(_long_row(r, b.used))
    b.short(4)
    b.add(b"what is your social security number", agent=True)
    return b.rows


def test_cut_row_opens_and_closes_the_gate(compiled, oracle_cfg):
    """gate closed: ERR_LONG on the cut row, the re-run with the long-row kernels (lanes cut at both
    ends, no row start inside); gate open: cut lanes in every call; then closed again"""
    es = _engines(compiled.blob)
    try:
        r = random.Random(40)
        b = _slots(600)
        rows = _Rows(r, b)
        rows.short(20)
        _, st = _check(es, rows.rows, oracle_cfg)
        assert _closed(st)
        _, st = _check(es, _long_batch(r, b + 40), oracle_cfg)
        assert st["cut_rows"] >= 1 and (st["long_kernels_launched"], st["reruns"]) == (1, 1)
        _, st = _check(es, _long_batch(r, b + 80), oracle_cfg)
        assert st["cut_rows"] >= 1 and (st["long_kernels_launched"], st["reruns"]) == (1, 0)
        for k in range(LONG_IDLE_CALLS):
            rows = _Rows(r, b + 120 + 20 * k)
            rows.short(9)
            _, st = _check(es, rows.rows, oracle_cfg)
            assert (st["cut_rows"], st["long_kernels_launched"], st["reruns"]) == (0, 1, 0), k
        _, st = _check(es, _boundary_rows(r, b + 400), oracle_cfg)
        assert _closed(st)
        _, st = _check(es, _long_batch(r, b + 500), oracle_cfg)
        assert st["cut_rows"] >= 1 and (st["long_kernels_launched"], st["reruns"]) == (1, 1)
    finally:
        for e in es:
            e.close()


# ------------------------------------------------ the window re-scan: no row is ever cut (NO_CUTS)
def test_window_rescan_with_every_length_bucket(compiled, oracle_cfg):
    """one incremental window re-scan call, one row per conversation: rows up to 4.2 KB stay whole, so
    lanes of every one of the 128 length buckets are sorted, and long lanes take the word slow path"""
    from oracle import pii_oracle as O
    r = random.Random(50)
    b = _Rows(r, 0)
    # rows of at least a slice each, one behind the other: each is the only one starting in its slice,
    # so its lane is as long as the row ...
    for m in range(4, LANE_NB + 3):
        n = 32 * m + r.randrange(32)
        b.add(_sparse(r, n) if m % 3 else _fill(n))
    # ... and short rows between such rows: a lane of its own wherever the next row starts in a later slice
    for _ in range(40):
        b.add(_fill(r.randrange(LANE, 3 * LANE)))
        b.add(_dense(r, r.randrange(33, LANE)))
    b.add(b"")
    b.add(b"my card is 4111 1111 1111 1111")
    lens = _lane_lengths(b.rows)
    assert {min(n >> 5, LANE_NB - 1) for n in lens} == set(range(LANE_NB))
    rows = b.rows
    es = _engines(compiled.blob)
    try:
        got = []
        for e in es:
            e.window_enable(5, 8192)
            assert e.window_mode() == "incremental"
            res = e.rescan_window([t for _, _, t, _ in rows], [c for c, _, _, _ in rows], [x for _, x, _, _ in rows],
                                  [s for _, _, _, s in rows])
            st = e.stats()
            got.append((res, {k: st[k] for k in ("pairs", "events", "lanes", "lane_bytes", "spans")}))
        for res, st in got[:-1]:
            assert np.array_equal(res.out, got[-1][0].out)
            assert np.array_equal(res.out_offsets, got[-1][0].out_offsets)
            assert np.array_equal(res.spans, got[-1][0].spans)
            assert np.array_equal(res.ctx_info, got[-1][0].ctx_info)
            assert st == got[-1][1]
        res, st = got[0]
        assert st["lane_bytes"] == LANE and st["lanes"] == len(lens)
        exp = O.process_window_rows(rows, oracle_cfg, n=5, store=O.ContextStore(), history={})
        groups = list(oracle_cfg.context_keywords.keys())
        for i, (red, fs, et) in enumerate(exp):
            assert res.text(i) == red, i
            assert _spans(res, i) == [(f.start, f.end, f.type_id, f.likelihood) for f in fs], i
            g = int(res.ctx_info[i])
            assert (groups[g] if g >= 0 else None) == et, i
    finally:
        for e in es:
            e.close()
