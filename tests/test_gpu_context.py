"""The conversation context path on the GPU -- the keyword automaton K (k_scan, k_scan_fix), the group priority
(k_pairs_flat's atomicMin over kw[u], started from kw_always_min by k_chunk_index), the segmented scan
(k_ctx_scan / k_ctx_apply, ctx_carry across tiles, both load paths), the TTL test, the commit list and
k_ctx_commit, the stamp / epoch ORDER check and win_ctx -- against the oracle's replay (process_rows,
process_window_rows, ContextStore) on the case lists of context_cases.

Every row of every list is compared -- ctx_info, output bytes and spans -- and after every call context_get of
every slot (group and timestamp); none is sampled or skipped.  test_context_cases.py (no GPU) checks that the
lists reach what they claim to.  Needs an MI355X: pytest -m gpu."""
import numpy as np
import pytest

import context_cases as CC
from conftest import pkg

pytestmark = pytest.mark.gpu

N_SLOTS = CC.SLOTS
_ORACLE = {}           # (batch, variant of the replay) -> its oracle results: computed once, never changed


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


@pytest.fixture(scope="module")
def engines(rules):
    E = pkg("engine")
    made = {}

    def get(name):
        if name not in made:
            made[name] = E.Engine(rules[name][1].blob, device=0, n_conv_slots=N_SLOTS)
        return made[name]
    yield get
    for e in made.values():
        e.close()


# ------------------------------------------------------------------------------------------- helpers
def _cols(rows, ts=True):
    return ([r[2] for r in rows], [r[0] for r in rows], [r[1] for r in rows], [r[3] for r in rows] if ts else None)


def _gi(eng):
    gi = {t: g for g, t in enumerate(eng.group_types)}
    gi[None] = -1
    return gi


def _want_ctx(exp, rows, gi, window=False):
    if window:
        return [gi[x[2]] for x in exp]
    return [gi[x[3]] if r[1] == CC.AGENT else gi[x[2]] if r[1] == CC.CUSTOMER else -1 for x, r in zip(exp, rows)]


def _check_rows(res, exp, rows, gi, labels=None, outputs=True, window=False):
    """ctx_info of every row; with outputs, every row's bytes, the offsets and the span list"""
    ctx = res if isinstance(res, np.ndarray) else res.ctx_info
    got, want = [int(v) for v in ctx], _want_ctx(exp, rows, gi, window)
    assert len(got) == len(want)
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, (len(bad), [(i, labels[i] if labels else rows[i], got[i], want[i]) for i in bad[:5]])
    if not outputs:
        return
    for i, x in enumerate(exp):
        assert res.text(i) == x[0], (i, labels[i] if labels else rows[i], res.text(i), x[0])
    assert [int(o) for o in res.out_offsets] == [0] + list(np.cumsum([len(x[0]) for x in exp]))
    spans = [(int(s["utt"]), int(s["start"]), int(s["end"]), int(s["info_type"]), int(s["likelihood"])) for s in res.spans]
    assert spans == [(i, f.start, f.end, f.type_id, f.likelihood) for i, x in enumerate(exp) for f in x[1]]


def _snapshot(eng):
    return [eng.context_get(sl) for sl in range(eng.n_slots)]


def _check_store(eng, store, gi):
    """context_get of every slot: the record the oracle's store holds (group and timestamp), else none"""
    for sl, got in enumerate(_snapshot(eng)):
        v = store.d.get(sl)
        assert got == ((gi[v[0]], v[2]) if v else (-1, 0)), (sl, got, v)


def _preset(eng, store, recs):
    for sl, g, ts in recs:
        eng.context_set(sl, g, ts)
        store.set(sl, eng.group_types[g], b"", ts)


def _reset(eng, store):
    for sl in list(store.d):
        eng.context_set(sl, -1, 0)
    store.d.clear()


def _place(arr, shift):
    """arr `shift` elements into a device tensor: 16-byte aligned for shift 0, misaligned otherwise (as
    test_gpu_alignment.py places them); returns (owner, view)"""
    import torch
    arr = np.array(arr)                   # (a writable copy: frombuffer's arrays are not)
    t = torch.zeros(len(arr) + shift + 64, dtype=torch.from_numpy(arr[:0]).dtype, device="cuda:0")
    t[shift:shift + len(arr)] = torch.from_numpy(arr).to("cuda:0")
    return t, t[shift:]


class DevBatch:
    """rows in device memory for the device entry points.  shift: the per-row arrays (slot, role, ts, ctx) one
    element into their tensors (k_ctx_*'s scalar path) or 16-byte aligned (vector path); phase: the text's
    address mod 64; pre / post: bytes before the first row and after the last"""

    def __init__(self, rows, shift=0, phase=0, pre=b"", post=b"", ts=True):
        texts, slots, roles, tss = _cols(rows)
        self.n = len(rows)
        data = np.frombuffer(pre + b"".join(texts) + post, dtype=np.uint8)
        self.offs = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int64) + len(pre)
        self.keep = []
        own, self.text = _place(data if len(data) else np.zeros(1, np.uint8), phase)
        assert own.data_ptr() % 64 == 0 and self.text.data_ptr() % 64 == phase % 64
        self.keep.append(own)
        own, self.d_offs = _place(self.offs, 0)
        self.keep.append(own)
        own, self.slot = _place(np.asarray(slots, dtype=np.uint32).view(np.int32), shift)
        self.keep.append(own)
        own, self.role = _place(np.asarray(roles, dtype=np.uint8), shift)
        self.keep.append(own)
        own, self.ts = _place(np.asarray(tss, dtype=np.int64), shift)
        self.keep.append(own)
        own, self.ctx = _place(np.full(self.n, -7, dtype=np.int16), shift)
        self.keep.append(own)
        self.with_ts = ts
        for t, a in ((self.slot, 16), (self.role, 8), (self.ts, 16), (self.ctx, 16)):
            assert (t.data_ptr() % a == 0) == (shift == 0)

    def call(self, eng, exp, i0=0, i1=None, out_cap=None):
        """rows [i0, i1) through pii_scan_redact_device_ex, the batch's base and size declared; exp sizes the
        output.  Returns the BatchResult after sync (which raises what the call failed with)."""
        import torch
        E = pkg("engine")
        i1 = self.n if i1 is None else i1
        n = i1 - i0
        if out_cap is None:
            out_cap = sum(len(x[0]) for x in exp) + 64
        span_cap = sum(len(x[1]) for x in exp) + 64
        d_out = torch.full((max(out_cap, 1) + 64,), 0xEE, dtype=torch.uint8, device="cuda:0")
        d_oo = torch.zeros(n + 1, dtype=torch.int64, device="cuda:0")
        d_sp = torch.zeros(span_cap * 16, dtype=torch.uint8, device="cuda:0")
        base, size = int(self.offs[i0]), int(self.offs[i1] - self.offs[i0])
        eng.scan_redact_device_ex(self.text.data_ptr(), self.d_offs.data_ptr() + 8 * i0, n, base, size,
                                  self.slot.data_ptr() + 4 * i0, self.role.data_ptr() + i0,
                                  self.ts.data_ptr() + 8 * i0 if self.with_ts else None, d_out.data_ptr(), out_cap,
                                  d_oo.data_ptr(), d_sp.data_ptr(), span_cap, self.ctx.data_ptr() + 2 * i0)
        ob, ns, flags = eng.sync()
        assert flags == 0
        assert int(d_out[out_cap:].min()) == 0xEE                      # nothing written past out_cap
        spans = np.frombuffer(d_sp[:ns * 16].cpu().numpy().tobytes(), dtype=E.SPAN_DTYPE)
        return E.BatchResult(d_out[:ob].cpu().numpy(), d_oo.cpu().numpy().astype(np.uint64), spans,
                             self.ctx[i0:i1].cpu().numpy())


def _oracle(key, rows, ocfg, recs=(), group_types=None, window=False):
    """(per-row results, the store after them) of the replay of `rows` after the preset records: computed once"""
    from oracle import pii_oracle as O
    if key not in _ORACLE:
        store = O.ContextStore()
        for sl, g, ts in recs:
            store.set(sl, group_types[g], b"", ts)
        exp = O.process_window_rows(rows, ocfg, n=5, store=store) if window else O.process_rows(rows, ocfg, store)
        _ORACLE[key] = (exp, dict(store.d))
    return _ORACLE[key]


# --------------------------------------------------------------------------------------- 1 keyword rows
def _keyword_batches(name):
    """[(batch name, rows, labels)]: the keyword texts as AGENT / CUSTOMER / OTHER rows of one conversation each,
    then the split rows' four variants, each batch with slots of its own"""
    kt = CC.keyword_texts(name)
    rows = CC.conversation_rows([t for _, t in kt])
    out = [("texts", rows, [label for label, _ in kt for _ in range(5)])]
    slot0 = len(kt)
    pairs = CC.split_pairs(name)
    for variant in ("one", "two", "empty", "wrap"):
        r = CC.split_rows(pairs, variant, slot0=slot0)
        slot0 = max(x[0] for x in r) + 1
        out.append((variant, r, None))
    assert slot0 <= N_SLOTS
    return out


@pytest.mark.parametrize("call", ["scan_redact", "context_update"])
@pytest.mark.parametrize("name", CC.FILES)
def test_keyword_and_split_rows(name, call, rules, engines):
    from oracle import pii_oracle as O
    ocfg, eng = rules[name][0], engines(name)
    gi = _gi(eng)
    store = O.ContextStore()
    stored = 0
    for bname, rows, labels in _keyword_batches(name):
        exp, after = _oracle((name, bname), rows, ocfg)
        if bname == "wrap":               # batches of two rows: the second half first, the first half last
            fn = eng.scan_redact if call == "scan_redact" else eng.context_update
            for i in range(0, len(rows), 2):
                _check_rows(fn(*_cols(rows[i:i + 2])), exp[i:i + 2], rows[i:i + 2], gi, outputs=call == "scan_redact")
        elif call == "scan_redact":
            res = eng.scan_redact(*_cols(rows))
            _check_rows(res, exp, rows, gi, labels)
        else:
            ctx = eng.context_update(*_cols(rows))
            _check_rows(ctx, exp, rows, gi, labels, outputs=False)
        store.d.update(after)
        _check_store(eng, store, gi)
        stored += len(after)
        if bname != "texts" and name == "shipped":
            # most halves store nothing: their slots stay empty
            assert len(after) < len({r[0] for r in rows}) // 2
    assert stored > 1000
    _reset(eng, store)


@pytest.mark.parametrize("name", CC.FILES)
def test_split_rows_with_the_other_half_outside_the_batch(name, rules, engines):
    """the device entry point over sub-ranges of one buffer: every call's batch_base is non-zero, its first row is
    a second half whose first half ends right before batch_base, and its last row a first half whose second half
    begins at the batch's end"""
    from oracle import pii_oracle as O
    ocfg, eng = rules[name][0], engines(name)
    gi = _gi(eng)
    pairs = CC.split_pairs(name)
    rows = CC.split_rows(pairs, "two")
    assert len({r[0] for r in rows}) == len(rows) <= N_SLOTS
    exp, after = _oracle((name, "two at slot 0"), rows, ocfg)
    dev = DevBatch(rows, shift=0, phase=5)
    called = set()
    texts = [r[2] for r in rows]
    step = 64
    for i0 in range(1, len(rows) - 1, step):
        i1 = min(i0 + step, len(rows) - 1)
        i1 -= (i1 - i0) % 2                                           # an even count: ends with a first half
        if i1 <= i0:
            break
        assert i0 % 2 == 1 and rows[i0 - 1][2] + rows[i0][2] == pairs[i0 // 2][1] + pairs[i0 // 2][2]
        assert rows[i1 - 1][2] + rows[i1][2] == pairs[i1 // 2][1] + pairs[i1 // 2][2]
        assert int(dev.offs[i0]) > 0 and b"".join(texts[:i0]).endswith(rows[i0 - 1][2])
        res = dev.call(eng, exp[i0:i1], i0, i1)
        _check_rows(res, exp[i0:i1], rows[i0:i1], gi)
        called |= {r[0] for r in rows[i0:i1]}
    assert len(called) >= len(rows) - 66
    store = O.ContextStore()
    store.d.update({sl: v for sl, v in after.items() if sl in called})
    _check_store(eng, store, gi)
    _reset(eng, store)


@pytest.mark.parametrize("name", CC.FILES)
def test_keyword_and_split_rows_on_the_device_path(name, rules, engines):
    """the keyword texts and the split rows of one conversation (with and without the empty row between) through
    the device entry point over sub-ranges of one buffer whose text lies 9 bytes off a 64-byte boundary behind half
    a keyword: every call's batch_base is non-zero.  The split rows' calls begin with the second half -- the first
    half, a row of the same conversation, ends right before batch_base (for 'empty': before the empty row that
    ends there) -- and end with a first half whose second half begins at the batch's end"""
    from oracle import pii_oracle as O
    ocfg, eng = rules[name][0], engines(name)
    gi = _gi(eng)
    store = O.ContextStore()
    kw = CC.keywords_of(name)[0][2]
    for bname, rows, labels in _keyword_batches(name):
        if bname in ("two", "wrap"):            # 'two': test_split_rows_with_the_other_half_outside_the_batch
            continue
        exp, after = _oracle((name, bname), rows, ocfg)
        dev = DevBatch(rows, shift=0, phase=9, pre=b"- " + kw[:2], post=kw[2:] + b" -")
        first, step = {"texts": (0, 997), "one": (1, 64), "empty": (2, 63)}[bname]
        cuts = sorted({0, len(rows)} | set(range(first, len(rows), step)))
        for i0, i1 in zip(cuts, cuts[1:]):
            assert int(dev.offs[i0]) > 0
            if bname == "one" and i0:
                assert rows[i0 - 1][0] == rows[i0][0] and rows[i0 - 1][2] + rows[i0][2] == b"".join(CC.split_pairs(name)[i0 // 2][1:])
            if bname == "empty" and i0:
                assert rows[i0 - 1][2] == b"" and rows[i0 - 2][0] == rows[i0][0]
                assert rows[i0 - 2][2] + rows[i0][2] == b"".join(CC.split_pairs(name)[i0 // 3][1:])
            res = dev.call(eng, exp[i0:i1], i0, i1)
            _check_rows(res, exp[i0:i1], rows[i0:i1], gi, labels[i0:i1] if labels else None)
        store.d.update(after)
        _check_store(eng, store, gi)
    _reset(eng, store)


# ------------------------------------------------------------------------------------- 2 lane-cut rows
def _lane_batch(name, r0, lane=128, every=1):
    lane_rows, where = CC.lane_rows(name, r0=r0, lane=lane, every=every)
    rows = [(i % N_SLOTS, CC.AGENT, r, CC.T0 + i) for i, (_, r) in enumerate(lane_rows)]
    return rows, [label for label, _ in lane_rows]


@pytest.mark.parametrize("name", CC.FILES)
def test_lane_cut_rows_on_the_host_path(name, rules, engines):
    from oracle import pii_oracle as O
    ocfg, eng = rules[name][0], engines(name)
    gi = _gi(eng)
    rows, labels = _lane_batch(name, 0)
    assert len(rows) <= N_SLOTS
    exp, after = _oracle((name, "lane", 0), rows, ocfg)
    res = eng.scan_redact(*_cols(rows))
    st = eng.stats(gate=True)
    # the geometry the rows were built for: 128-byte lanes, and every row (all are longer than two lanes) cut
    assert st["lane_bytes"] == 128 and st["cut_rows"] == len(rows) and st["long_kernels_launched"] == 1, st
    _check_rows(res, exp, rows, gi, labels)
    miss = gi[CC.miss_type(name)]
    hits = sum(int(v) != miss for v in res.ctx_info)
    assert len(rows) // 3 < hits < 2 * len(rows) // 3 + 50          # the rows hit, (most of) their siblings do not
    store = O.ContextStore()
    store.d.update(after)
    _check_store(eng, store, gi)
    ctx = eng.context_update(*_cols(rows))
    _check_rows(ctx, exp, rows, gi, labels, outputs=False)
    _reset(eng, store)


@pytest.mark.parametrize("phase", [7, 48])
@pytest.mark.parametrize("name", CC.FILES)
def test_lane_cut_rows_on_the_device_path(name, phase, rules, engines):
    """the text at an address of `phase` mod 64: the cuts are counted from it (r0)"""
    from oracle import pii_oracle as O
    ocfg, eng = rules[name][0], engines(name)
    gi = _gi(eng)
    rows, labels = _lane_batch(name, phase)
    exp, after = _oracle((name, "lane", phase), rows, ocfg)
    res = DevBatch(rows, shift=0, phase=phase).call(eng, exp)
    st = eng.stats(gate=True)
    assert st["lane_bytes"] == 128 and st["cut_rows"] == len(rows) and st["long_kernels_launched"] == 1, st
    _check_rows(res, exp, rows, gi, labels)
    store = O.ContextStore()
    store.d.update(after)
    _check_store(eng, store, gi)
    _reset(eng, store)


def test_lane_cut_rows_at_256_byte_lanes(rules, engines):
    """the second lane size: 16 MiB of batch give 256-byte lanes (65536 lanes on the MI355X's 256 CUs).  The batch is
    padded with copies of one filler row of 250 bytes (never cut), whose oracle result is computed once"""
    from oracle import pii_oracle as O
    ocfg, eng = rules["shipped"][0], engines("shipped")
    gi = _gi(eng)
    rows, labels = _lane_batch("shipped", 0, lane=256, every=3)
    filler = CC.fill(250, 1)
    n_fill = ((17 << 20) - sum(len(r[2]) for r in rows)) // len(filler)
    exp, after = _oracle(("shipped", "lane256"), rows, ocfg)
    fexp = O.process_rows([(N_SLOTS - 1, CC.OTHER, filler, 0)], ocfg)[0]
    assert fexp[0] == filler and not fexp[1]
    texts, slots, roles, ts = _cols(rows)
    res = eng.scan_redact(texts + [filler] * n_fill, slots + [N_SLOTS - 1] * n_fill, roles + [CC.OTHER] * n_fill,
                          ts + [0] * n_fill)
    st = eng.stats(gate=True)
    assert st["lane_bytes"] == 256 and st["cut_rows"] == len(rows), st
    n = len(rows)
    want = _want_ctx(exp, rows, gi)
    assert [int(v) for v in res.ctx_info[:n]] == want and (res.ctx_info[n:] == -1).all()
    for i, x in enumerate(exp):
        assert res.text(i) == x[0], labels[i]
    tail = res.out[int(res.out_offsets[n]):]
    assert len(tail) == n_fill * len(filler) and (tail.reshape(n_fill, len(filler)) == np.frombuffer(filler, np.uint8)).all()
    assert len(res.spans) == sum(len(x[1]) for x in exp)
    store = O.ContextStore()
    store.d.update(after)
    _check_store(eng, store, gi)
    _reset(eng, store)


# ------------------------------------------------------------------------------ 3 run-structure batches
def _batch(name):
    if name == "edges":
        return CC.edge_batch()
    if name.startswith("n="):
        return CC.edge_batch()[:int(name[2:])]
    return CC.long_batch(name == "long-sibling")


def _recs(name, rows, eng):
    """the records set before the batch: edges -- a third of its slots, CVV, live for the batch's first half; long
    batches -- every slot, SSN, live throughout (the hit must override it, the sibling must read it)"""
    gi = _gi(eng)
    if name.startswith("long"):
        return [(sl, gi["US_SOCIAL_SECURITY_NUMBER"], CC.T0 - 1000) for sl in sorted({r[0] for r in rows})]
    return CC.presets(rows, gi["CVV_NUMBER"])


MODES = ["scan_redact", "context_update", "device-vector", "device-scalar", "no-timestamps"]


def _run_mode(eng, ocfg, name, mode, gi):
    """one batch through one call, compared with the oracle's replay; leaves the engine's records reset"""
    from oracle import pii_oracle as O
    rows = _batch(name)
    recs = _recs(name, rows, eng)
    if mode == "no-timestamps":
        rows = [(r[0], r[1], r[2], 0) for r in rows]          # ts = NULL: the replay in which every timestamp is 0
    exp, after = _oracle((name, mode == "no-timestamps"), rows, ocfg, recs, eng.group_types)
    store = O.ContextStore()
    _preset(eng, store, recs)
    if mode == "scan_redact":
        _check_rows(eng.scan_redact(*_cols(rows)), exp, rows, gi)
    elif mode == "context_update":
        _check_rows(eng.context_update(*_cols(rows)), exp, rows, gi, outputs=False)
    elif mode == "no-timestamps":
        _check_rows(eng.scan_redact(*_cols(rows, ts=False)), exp, rows, gi)
    else:
        dev = DevBatch(rows, shift=0 if mode == "device-vector" else 1)
        _check_rows(dev.call(eng, exp), exp, rows, gi)
    store.d.clear()
    store.d.update(after)
    _check_store(eng, store, gi)
    _reset(eng, store)
    return exp


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["edges", "long", "long-sibling"])
def test_run_structure_batches(name, mode, rules, engines):
    ocfg, eng = rules[CC.RUN_FILE][0], engines(CC.RUN_FILE)
    gi = _gi(eng)
    exp = _run_mode(eng, ocfg, name, mode, gi)
    rows = _batch(name)
    used = {x[2] for x, r in zip(exp, rows) if r[1] == CC.CUSTOMER}
    if name == "long":          # the third tile's customers use the hit of row 1, two tiles back
        assert used == {"CVV_NUMBER"}
    elif name == "long-sibling":   # ... and the sibling's its own record, not that hit
        assert used == {"US_SOCIAL_SECURITY_NUMBER"}
    else:
        want = {None, "CVV_NUMBER", "US_SOCIAL_SECURITY_NUMBER", "DATE_OF_BIRTH"}
        assert used == want


@pytest.mark.parametrize("mode", MODES)
def test_row_counts_around_the_group_sizes(mode, rules, engines):
    """n_utt around a thread's 8, a wavefront's 512 and a tile's 2048 rows: the full / tail split of ctx_load and
    of the packed stores changes sides"""
    ocfg, eng = rules[CC.RUN_FILE][0], engines(CC.RUN_FILE)
    gi = _gi(eng)
    for n in CC.N_UTT:
        _run_mode(eng, ocfg, "n=%d" % n, mode, gi)


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("name", ["edges", "long", "long-sibling"])
def test_run_structure_batches_on_the_window_path(name, full, rules):
    """win_ctx: the context a request right after the row would get, and the windows redacted under it"""
    from oracle import pii_oracle as O
    E = pkg("engine")
    ocfg, comp = rules[CC.RUN_FILE]
    eng = E.Engine(comp.blob, device=0, n_conv_slots=N_SLOTS)
    try:
        eng.window_enable(5, 1024, full=full)
        assert int(comp.sections["meta"][13]) == 1          # the rules allow the incremental re-scan
        assert eng.window_mode() == ("full" if full else "incremental")
        gi = _gi(eng)
        rows = _batch(name)
        recs = _recs(name, rows, eng)
        exp, after = _oracle((name, "window"), rows, ocfg, recs, eng.group_types, window=True)
        store = O.ContextStore()
        _preset(eng, store, recs)
        res = eng.rescan_window(*_cols(rows))
        _check_rows(res, exp, rows, gi, window=True)
        assert sum(len(x[1]) for x in exp) > 100
        store.d.clear()
        store.d.update(after)
        _check_store(eng, store, gi)
    finally:
        eng.close()


@pytest.mark.parametrize("full", [False, True])
def test_row_counts_and_ttl_on_the_window_path(full, rules):
    """win_ctx at n_utt around 8, 512 and 2048 -- the full / tail split of its packed store -- and at ttl - 1, ttl and
    ttl + 1 microseconds, with the windows redacted under it"""
    from oracle import pii_oracle as O
    E = pkg("engine")
    ocfg, comp = rules[CC.RUN_FILE]
    assert int(comp.sections["meta"][13]) == 1
    eng = E.Engine(comp.blob, device=0, n_conv_slots=N_SLOTS)
    try:
        eng.window_enable(5, 1024, full=full)
        assert eng.window_mode() == ("full" if full else "incremental")
        gi = _gi(eng)
        store = O.ContextStore()
        for n in CC.N_UTT:
            name = "n=%d" % n
            rows = _batch(name)
            recs = _recs(name, rows, eng)
            exp, after = _oracle((name, "window"), rows, ocfg, recs, eng.group_types, window=True)
            _preset(eng, store, recs)
            res = eng.rescan_window(*_cols(rows))
            assert len(res.ctx_info) == n
            _check_rows(res, exp, rows, gi, window=True)
            store.d.clear()
            store.d.update(after)
            _check_store(eng, store, gi)
            for sl in {r[0] for r in rows}:
                eng.window_reset(sl)
            _reset(eng, store)
        one, two = CC.ttl_batch()
        _preset(eng, store, [(CC.slot_of(10 + k), gi["CVV_NUMBER"], CC.T0) for k in range(3)])
        hist = {}
        for rows in (one, two):
            exp = O.process_window_rows(rows, ocfg, n=5, store=store, history=hist)
            _check_rows(eng.rescan_window(*_cols(rows)), exp, rows, gi, window=True)
            _check_store(eng, store, gi)
            assert {x[2] for x in exp} >= {None, "CVV_NUMBER"}
    finally:
        eng.close()


@pytest.mark.parametrize("mode", MODES[:4])
def test_ttl_at_the_microsecond(mode, rules, engines):
    """ttl - 1, ttl and ttl + 1 microseconds after a hit of the same run, after a record set from outside and
    after a record an earlier call stored; the committed timestamp is the hit's, not the run's last row's"""
    from oracle import pii_oracle as O
    ocfg, eng = rules[CC.RUN_FILE][0], engines(CC.RUN_FILE)
    gi = _gi(eng)
    one, two = CC.ttl_batch()
    recs = [(CC.slot_of(10 + k), gi["CVV_NUMBER"], CC.T0) for k in range(3)]
    store = O.ContextStore()
    _preset(eng, store, recs)
    for k, rows in enumerate((one, two)):
        exp = O.process_rows(rows, ocfg, store)
        if mode == "scan_redact":
            _check_rows(eng.scan_redact(*_cols(rows)), exp, rows, gi)
        elif mode == "context_update":
            _check_rows(eng.context_update(*_cols(rows)), exp, rows, gi, outputs=False)
        else:
            _check_rows(DevBatch(rows, shift=0 if mode == "device-vector" else 1).call(eng, exp), exp, rows, gi)
        _check_store(eng, store, gi)
        used = [x[2] for x, r in zip(exp, rows) if r[1] == CC.CUSTOMER]
        assert None in used and "CVV_NUMBER" in used
    for k in range(3):                                               # the hits' timestamps, 50 s before the last rows'
        assert eng.context_get(CC.slot_of(20 + k)) == (gi["CVV_NUMBER"], CC.T0 + 10 + k)
    _reset(eng, store)


# ------------------------------------------------------------------------------------- 4 persistence
def test_a_batch_split_into_calls_equals_the_single_call(rules, engines):
    from oracle import pii_oracle as O
    ocfg, eng = rules[CC.RUN_FILE][0], engines(CC.RUN_FILE)
    gi = _gi(eng)
    rows = _batch("edges")
    recs = _recs("edges", rows, eng)
    exp, after = _oracle(("edges", False), rows, ocfg, recs, eng.group_types)
    hit = {t: O.extract_expected_pii(t, ocfg) for t in {r[2] for r in rows}}
    same = [i for i in range(1, len(rows)) if rows[i][0] == rows[i - 1][0]]
    after_hit = [i for i in same if rows[i - 1][1] == CC.AGENT and hit[rows[i - 1][2]] and rows[i][1] == CC.CUSTOMER]
    inside = [i for i in same if rows[i][1] == CC.CUSTOMER and not (rows[i - 1][1] == CC.AGENT and hit[rows[i - 1][2]])]
    cuts = sorted({after_hit[0], inside[len(inside) // 7], after_hit[len(after_hit) // 2], inside[len(inside) // 2],
                   2048, after_hit[-1], inside[-1]})
    assert len(cuts) >= 6
    single = None
    for parts in ([0, len(rows)], [0] + cuts + [len(rows)]):
        store = O.ContextStore()
        _preset(eng, store, recs)
        got = []
        for a, b in zip(parts, parts[1:]):
            res = eng.scan_redact(*_cols(rows[a:b]))
            _check_rows(res, exp[a:b], rows[a:b], gi)
            got += [(int(c), res.text(i)) for i, c in enumerate(res.ctx_info)]
        single = single or got
        assert got == single
        store.d.clear()
        store.d.update(after)
        _check_store(eng, store, gi)
        _reset(eng, store)


# ------------------------------------------------------------------------------ 5 nothing on failure
def _one_row_runs(rows):
    return [i for i in range(1, len(rows) - 1) if rows[i - 1][0] != rows[i][0] != rows[i + 1][0]]


@pytest.mark.parametrize("failure", ["slot", "order", "capacity"])
def test_a_failed_call_commits_nothing_and_the_next_call_is_clean(failure, rules, engines):
    from oracle import pii_oracle as O
    E = pkg("engine")
    ocfg, eng = rules[CC.RUN_FILE][0], engines(CC.RUN_FILE)
    gi = _gi(eng)
    rows = _batch("edges")[:5000]
    recs = _recs("edges", rows, eng)
    store = O.ContextStore()
    _preset(eng, store, recs)
    before = _snapshot(eng)
    ones = _one_row_runs(rows)
    bad = list(rows)
    if failure == "slot":                     # a slot equal to n_conv_slots
        k = next(i for i in ones if i > 500)
        bad[k] = (N_SLOTS,) + rows[k][1:]
        code = E.PII_E_ARG
    elif failure == "order":                  # one slot in two runs that lie in different tiles
        k0, k = ones[0], next(i for i in ones if i >= 4096)
        assert k0 < 2048 and rows[k0][0] != rows[k][0]
        bad[k] = (rows[k0][0],) + rows[k][1:]
        code = E.PII_E_ORDER
    if failure == "capacity":                 # a device call whose out_cap is too small
        exp, after = _oracle(("edges", 5000), rows, ocfg, recs, eng.group_types)
        dev = DevBatch(rows)
        with pytest.raises(E.PiiError) as ei:
            dev.call(eng, exp, out_cap=sum(len(x[0]) for x in exp) // 2)
        assert ei.value.code == E.PII_E_CAPACITY
        assert _snapshot(eng) == before
        _check_rows(dev.call(eng, exp), exp, rows, gi)
    else:
        for attempt in ("scan_redact", "context_update"):
            with pytest.raises(E.PiiError) as ei:
                getattr(eng, attempt)(*_cols(bad))
            assert ei.value.code == code
            assert _snapshot(eng) == before
        rows = bad[:k] + bad[k + 1:]          # the offending row dropped
        exp, after = _oracle(("edges", 5000, failure), rows, ocfg, recs, eng.group_types)
        _check_rows(eng.scan_redact(*_cols(rows)), exp, rows, gi)
    store.d.clear()
    store.d.update(after)
    _check_store(eng, store, gi)
    _reset(eng, store)


# -------------------------------------------------------------------------------- 6 the re-run by sync
def test_first_call_with_a_cut_row_is_run_again_by_sync(rules):
    """a fresh engine launches no long-row kernels; its first call holds a cut row among conversations of several
    rows, is void (ERR_LONG) and is run again by the wait -- with a new epoch, so that the slots the void run
    stamped are no ORDER error, and with nothing committed twice"""
    from oracle import pii_oracle as O
    E = pkg("engine")
    ocfg, comp = rules[CC.RUN_FILE]
    eng = E.Engine(comp.blob, device=0, n_conv_slots=N_SLOTS)
    try:
        gi = _gi(eng)
        rows = _batch("edges")[:600]
        k = next(i for i in range(100, 600) if rows[i][1] == CC.AGENT and rows[i][2] == CC.H_CVV and
                 rows[i + 1][0] == rows[i][0] and rows[i + 1][1] == CC.CUSTOMER)
        rows[k] = (rows[k][0], CC.AGENT, CC.fill(250, 2) + CC.H_CVV + CC.fill(150, 5), rows[k][3])
        exp = O.process_rows(rows, ocfg)
        res = eng.scan_redact(*_cols(rows))
        st = eng.stats(gate=True)
        assert st["reruns"] >= 1 and st["cut_rows"] == 1 and st["long_kernels_launched"] == 1, st
        _check_rows(res, exp, rows, gi)
        assert int(res.ctx_info[k]) == gi["CVV_NUMBER"] == int(res.ctx_info[k + 1])
        store = O.ContextStore()
        O.process_rows(rows, ocfg, store)
        _check_store(eng, store, gi)
    finally:
        eng.close()


# ----------------------------------------------------------------------------------- 7 context_resize
def test_context_resize_keeps_records_and_opens_empty_slots(rules):
    from oracle import pii_oracle as O
    E = pkg("engine")
    ocfg, comp = rules[CC.RUN_FILE]
    half = N_SLOTS // 2
    eng = E.Engine(comp.blob, device=0, n_conv_slots=half)
    try:
        gi = _gi(eng)
        rows = _batch("edges")[:3000]
        assert max(r[0] for r in rows) < half
        store = O.ContextStore()
        exp = O.process_rows(rows, ocfg, store)
        _check_rows(eng.scan_redact(*_cols(rows)), exp, rows, gi)
        before = _snapshot(eng)
        assert sum(g >= 0 for g, _ in before) > 10
        with pytest.raises(E.PiiError):
            eng.scan_redact([b"x"], [half], [CC.AGENT], [CC.T0])
        eng.context_resize(N_SLOTS)
        now = _snapshot(eng)
        assert now[:half] == before and now[half:] == [(-1, 0)] * half
        # old and new slots in one batch, the old ones reading the records stored before the resize
        more = [(r[0] + (half if (r[0] // 37) % 2 else 0), r[1], r[2], r[3] + 7_000_000) for r in _batch("edges")[3000:]]
        more = [(r[0], CC.CUSTOMER, CC.VALUE, r[3]) if i % 50 == 0 else r for i, r in enumerate(more)]
        assert {r[0] >= half for r in more} == {True, False}
        exp = O.process_rows(more, ocfg, store)
        _check_rows(eng.scan_redact(*_cols(more)), exp, more, gi)
        _check_store(eng, store, gi)
    finally:
        eng.close()
