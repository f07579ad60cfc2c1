"""External candidates on the window re-scan (pii_rescan_window_ext / _device_ext) on the GPU against
tests/window_ext_ref.py: redacted window bytes, window spans and window context group, bit-exact, in the
incremental mode (whole rows, the inline halo path, rows cut at one lane) and in the full re-scan.

A row's candidates are given once, with the row; every later window that holds the row must still redact
them -- from the history ring -- and a window that no longer holds the row must not."""
import contextlib
import functools
import os
import random

import numpy as np
import pytest

from conftest import pkg
from window_ext_stub import StubNer

import window_ext_ref as WR
import xform_configs as X
import xform_ref

pytestmark = pytest.mark.gpu

MODES = ["incremental", "full", "incremental_inline_halo", "incremental_cut1"]
_WENV = {"incremental_inline_halo": {"PII_HALO_ITEMS": "0"}, "incremental_cut1": {"PII_WIN_LONG": "1"}}


@contextlib.contextmanager
def _engine(blob, mode, slot_bytes=8192, n_slots=4096):
    """a fresh engine in `mode` (its environment is read at create) with window_enable(5, slot_bytes)"""
    E = pkg("engine")
    env = _WENV.get(mode, {})
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        e = E.Engine(blob, device=0, n_conv_slots=n_slots)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        e.window_enable(5, slot_bytes, full=mode == "full")
        assert e.window_mode() == ("full" if mode == "full" else "incremental")
        yield e
    finally:
        e.close()


@pytest.fixture(scope="module", params=MODES)
def weng(compiled, request):
    with _engine(compiled.blob, request.param) as e:
        e.mode = request.param
        yield e


def _spans_of(res, i):
    m = res.spans["utt"] == i
    return [(int(s["start"]), int(s["end"]), int(s["info_type"]), int(s["likelihood"])) for s in res.spans[m]]


def _compare(res, exp, cfg, rows):
    groups = list(cfg.context_keywords.keys())
    for i, (red, fs, et) in enumerate(exp):
        assert res.text(i) == red, (i, rows[i], res.text(i), red)
        assert _spans_of(res, i) == [(f.start, f.end, f.type_id, f.likelihood) for f in fs], (i, rows[i])
        g = int(res.ctx_info[i])
        assert (groups[g] if g >= 0 else None) == et, (i, rows[i])


def _check(eng, cfg, rows, ext, state, plain=False):
    """one call (rows: conv slot, role, text, ts) against the helper; plain: through rescan_window without
    the ext argument (every list must then be empty).  state: (ContextStore, history) of the helper"""
    args = ([t for _, _, t, _ in rows], [c for c, _, _, _ in rows], [r for _, r, _, _ in rows],
            [s for _, _, _, s in rows])
    if plain:
        assert not any(ext)
        res = eng.rescan_window(*args)
    else:
        res = eng.rescan_window(*args, ext=ext)
    exp = WR.process_window_rows_ext(rows, ext, cfg, n=5, store=state[0], history=state[1])
    _compare(res, exp, cfg, rows)
    return exp


def _state():
    from oracle import pii_oracle as O
    return O.ContextStore(), {}


# ----------------------------------------------------------------------------- the random streams
def _stream(cfg, seed, n_conv, per_conv):
    """conversations of the config-2 generator with names spliced in; per row, candidates in the manner of
    test_ner_redaction._random_ext: the name after "my name is", other types, 1-byte spans, spans
    overlapping each other and the rule findings, likelihoods below the minimum -- sorted by start"""
    from oracle import pii_oracle as O
    synth = pkg("synth")
    P = cfg.type_id["PERSON_NAME"]
    others = [cfg.type_id[x] for x in ("EMAIL_ADDRESS", "PHONE_NUMBER", "SOCIAL_HANDLE", "US_PASSPORT")]
    r = random.Random(seed)
    bank = synth.build_bank(300, 300, seed=seed)
    per = {}
    for c in range(n_conv):
        for j in range(per_conv):
            role = O.ROLE_AGENT if j % 2 == 0 else O.ROLE_CUSTOMER
            text = r.choice(bank.texts[:300] if role == O.ROLE_AGENT else bank.texts[300:])
            xs = []
            if r.random() < 0.4:
                name = f"{r.choice(synth.NAMES).capitalize()} {r.choice(synth.NAMES).capitalize()}"
                text = f"my name is {name}. ".encode() + text
                xs.append((11, 11 + len(name), P, 4))
            L = len(text)
            for _ in range(r.randrange(0, 4) if L else 0):
                s = r.randrange(0, L)
                e = min(L, s + r.choice([1, 2, 5, 9, 14, 30]))
                xs.append((s, e, P if r.random() < 0.7 else r.choice(others), r.choice([2, 3, 4, 4, 5])))
            xs.sort(key=lambda x: x[0])
            per.setdefault(c + 1, []).append(((c + 1, role, text, 1_760_000_000_000_000 + j * 5_000_000), xs))
    return per


def _overlap(a, b):
    return a[0] < b[1] and b[0] < a[1]


@functools.lru_cache(maxsize=None)
def _streamed_reference():
    """test 1's calls and the helper's answers, computed once for every mode: [(rows, ext, exp)]"""
    from oracle import pii_oracle as O
    cfg = O.RuleConfig.load()
    per = _stream(cfg, seed=41, n_conv=40, per_conv=12)
    state = _state()
    calls, kept, wins, loses, windows = [], 0, 0, 0, 0
    for k in range(12):
        rows = [per[c][k][0] for c in sorted(per)]
        ext = [per[c][k][1] for c in sorted(per)]
        exp = WR.process_window_rows_ext(rows, ext, cfg, n=5, store=state[0], history=state[1])
        calls.append((rows, ext, exp))
        for (c, _, _, _), (_, fs, et) in zip(rows, exp):
            text, joined = WR.join_extras(state[1][c])
            got = [(f.start, f.end, f.type_id, f.likelihood) for f in fs]
            plain = [(f.start, f.end, f.type_id, f.likelihood) for f in O.find_pii(text, cfg, et)]
            ext_kept = [f for f in got if f in joined and f not in plain]
            rule_kept = [f for f in got if f in plain and f not in joined]
            windows += 1
            kept += bool(ext_kept)
            # a candidate wins: it is kept and a rule finding of the candidate-free window overlapping it is gone
            wins += any(_overlap(x, p) and p not in got for x in ext_kept for p in plain)
            # a candidate loses: likely enough, not kept, and a kept rule finding overlaps it
            loses += any(x[3] >= 3 and x not in got and any(_overlap(x, f) for f in rule_kept) for x in joined)
    return calls, (windows, kept, wins, loses)


def _shift(rows, base):
    return [(c + base, r, t, s) for c, r, t, s in rows]


def test_streamed_one_row_per_conversation(weng, oracle_cfg):
    """40 conversations x 12 calls, every call the next row of every conversation with its candidates"""
    calls, (windows, kept, wins, loses) = _streamed_reference()
    assert windows == 480 and 3 * kept >= windows and wins >= 1 and loses >= 1, (windows, kept, wins, loses)
    for rows, ext, exp in calls:
        res = weng.rescan_window([t for _, _, t, _ in rows], [c for c, _, _, _ in rows], [r for _, r, _, _ in rows],
                                 [s for _, _, _, s in rows], ext=ext)
        _compare(res, exp, oracle_cfg, rows)


@functools.lru_cache(maxsize=None)
def _runs_reference():
    from oracle import pii_oracle as O
    cfg = O.RuleConfig.load()
    per = _stream(cfg, seed=53, n_conv=24, per_conv=17)
    rng = random.Random(5)
    state = _state()
    done = {c: 0 for c in per}
    calls = []
    while any(done[c] < len(per[c]) for c in per):
        batch = []
        for c in sorted(per):
            k = rng.choice([0, 1, 2, 3, 7])
            batch += per[c][done[c]:done[c] + k]
            done[c] = min(len(per[c]), done[c] + k)
        if batch:
            rows, ext = [b[0] for b in batch], [b[1] for b in batch]
            calls.append((rows, ext, WR.process_window_rows_ext(rows, ext, cfg, n=5, store=state[0],
                                                                 history=state[1])))
    return calls


def test_runs_within_a_batch(weng, oracle_cfg):
    """0, 1, 2, 3 or 7 rows of a conversation per call: windows mix resident and batch rows, some runs
    are longer than N"""
    calls = _runs_reference()
    assert any(sum(1 for r in rows if r[0] == rows[0][0]) > 5 for rows, _, _ in calls)
    for rows, ext, exp in calls:
        rows = _shift(rows, 100)
        res = weng.rescan_window([t for _, _, t, _ in rows], [c for c, _, _, _ in rows], [r for _, r, _, _ in rows],
                                 [s for _, _, _, s in rows], ext=ext)
        _compare(res, exp, oracle_cfg, rows)


# --------------------------------------------------------------------------------------- edges
def test_edges(weng, oracle_cfg):
    from oracle import pii_oracle as O
    A, C = O.ROLE_AGENT, O.ROLE_CUSTOMER
    P = oracle_cfg.type_id["PERSON_NAME"]
    EM = oracle_cfg.type_id["EMAIL_ADDRESS"]
    state = _state()
    rows = [
        # a candidate over an SSN whose hotword lies in the previous row: the halo bits of the rule record
        # and the marker of the external record meet at one start
        (900, C, b"please read me your social security", 1), (900, C, b"987654321 thanks", 2),
        (901, A, b"what is your email address", 1), (901, C, b"", 2),            # an empty row
        (901, C, b"Jane Doe", 3),                                                # a candidate over the whole row
        (901, C, b"I am Jane Doe", 4),                                           # ... ending at the row's last byte
        (901, C, b"jane.doe@example.com", 5), (901, C, b"jane.doe@example.com", 6),   # the email's own span: ties
        (901, C, b"jane.doe@example.com", 7), (901, C, b"ok", 8),
    ]
    ext = [[], [(0, 9, P, 4)], [], [], [(0, 8, P, 4)], [(5, 13, P, 5)],
           [(0, 20, P, 5)], [(0, 20, P, 1)], [(0, 20, EM, 5), (0, 20, P, 5)], []]
    exp = _check(weng, oracle_cfg, rows, ext, state)
    assert exp[4][0].endswith(b"\n[PERSON_NAME]") and exp[5][0].endswith(b"I am [PERSON_NAME]")
    assert weng.window_count(901) == 5
    # a call through the plain entry point: the resident names are still redacted
    exp = _check(weng, oracle_cfg, [(900, C, b"and my card 4141-1212-2323-5009", 3), (901, C, b"bye", 9)], [[], []],
                 state, plain=True)
    assert b"[PERSON_NAME]" in exp[1][0]
    # window_reset drops a conversation's candidates with its rows
    weng.window_reset(901)
    state[1].pop(901)
    exp = _check(weng, oracle_cfg, [(901, C, b"Jane Doe again", 10)], [[]], state)
    assert exp[0][0] == b"Jane Doe again"
    _check(weng, oracle_cfg, [], [], state)                                       # an empty batch
    _check(weng, oracle_cfg, [(905, C, b"", 1), (906, C, b"", 1)], [[], []], state)   # no scan lanes at all


@pytest.mark.parametrize("mode", MODES)
def test_ext_call_onto_rings_built_by_plain_calls(compiled, oracle_cfg, mode):
    """an engine that has never seen a candidate (its default kernels) builds the rings; the first _ext
    call then redacts its names and leaves the resident rule candidates in force"""
    from oracle import pii_oracle as O
    A, C = O.ROLE_AGENT, O.ROLE_CUSTOMER
    P = oracle_cfg.type_id["PERSON_NAME"]
    state = _state()
    with _engine(compiled.blob, mode, n_slots=64) as eng:
        rows = [(3, A, b"what is your social security number", 1), (3, C, b"987654321", 2), (4, C, b"hi there", 1)]
        _check(eng, oracle_cfg, rows, [[], [], []], state, plain=True)
        exp = _check(eng, oracle_cfg, [(3, C, b"my name is Ann Lee", 3), (4, C, b"Bob Ray here", 2)],
                     [[(11, 18, P, 4)], [(0, 7, P, 5)]], state)
        assert exp[0][0].endswith(b"my name is [PERSON_NAME]")
        assert [f.type_id == P for f in exp[0][1]] == [False, True]          # the resident rule finding, the name
        _check(eng, oracle_cfg, [(3, C, b"thanks", 4), (4, C, b"bye", 3)], [[], []], state, plain=True)


# --------------------------------------------------------------------------------- malformed lists
def test_malformed_lists_are_argument_errors_and_commit_nothing(weng, oracle_cfg):
    from oracle import pii_oracle as O
    E = pkg("engine")
    A, C = O.ROLE_AGENT, O.ROLE_CUSTOMER
    P = oracle_cfg.type_id["PERSON_NAME"]
    state = _state()
    _check(weng, oracle_cfg, [(950, C, b"hello there", 1)], [[(0, 5, P, 4)]], state)
    before = (weng.window_count(950), weng.context_get(950))
    texts = [b"What is your email address?", b"jane@example.com"]
    call = ([950, 950], [A, C], [2, 3])
    for bad in ([(5, 3, P, 4)], [(3, 3, P, 4)], [(0, 99, P, 4)], [(4, 6, P, 4), (1, 2, P, 4)], [(0, 2, 999, 4)],
                [(0, 2, P, 0)], [(0, 2, P, 6)]):
        with pytest.raises(E.PiiError) as ei:
            weng.rescan_window(texts, *call, ext=[[], bad])
        assert ei.value.code == E.PII_E_ARG, bad
        assert (weng.window_count(950), weng.context_get(950)) == before, bad
    # ext_n > ext_stride, a null pointer, stride 0: through the C entry point
    spans, counts, stride = E.ext_arrays([[], [(0, 4, P, 4)]], 2)
    counts[1] = stride + 1
    for fn in (lambda *a: weng.lib.pii_rescan_window_ext(*a, E._ptr(spans), E._ptr(counts), stride),
               lambda *a: weng.lib.pii_rescan_window_ext(*a, None, E._ptr(counts), stride),
               lambda *a: weng.lib.pii_rescan_window_ext(*a, E._ptr(spans), None, stride),
               lambda *a: weng.lib.pii_rescan_window_ext(*a, E._ptr(spans), E._ptr(counts), 0)):
        with pytest.raises(E.PiiError) as ei:
            weng._host_call(fn, "pii_rescan_window_ext", texts, *call, 5)
        assert ei.value.code == E.PII_E_ARG
        assert (weng.window_count(950), weng.context_get(950)) == before
    exp = _check(weng, oracle_cfg, [(950, A, texts[0], 2), (950, C, texts[1], 3)], [[], [(0, 4, P, 4)]], state)
    assert exp[1][0] == b"[PERSON_NAME] there\nWhat is your email address?\n[EMAIL_ADDRESS]"
    assert weng.window_count(950) == 3 and weng.group_types[weng.context_get(950)[0]] == "EMAIL_ADDRESS"


# ----------------------------------------------------------------------------------- ring capacity
@pytest.mark.parametrize("mode", MODES)
def test_candidates_count_against_the_ring_slot(compiled, oracle_cfg, mode):
    """window_enable(5, 256): a 100-byte row (112 B in the ring) with 12 candidates needs 192 + 112 > 256
    bytes -> PII_E_NOMEM, nothing committed; with 2 candidates it fits"""
    from oracle import pii_oracle as O
    E = pkg("engine")
    C = O.ROLE_CUSTOMER
    P = oracle_cfg.type_id["PERSON_NAME"]
    row = b"a" * 100
    with _engine(compiled.blob, mode, slot_bytes=256, n_slots=8) as eng:
        with pytest.raises(E.PiiError) as ei:
            eng.rescan_window([row], [1], [C], [1], ext=[[(8 * k, 8 * k + 3, P, 4) for k in range(12)]])
        assert ei.value.code == E.PII_E_NOMEM
        assert eng.window_count(1) == 0
        state = _state()
        _check(eng, oracle_cfg, [(1, C, row, 2)], [[(0, 3, P, 4), (50, 60, P, 4)]], state)
        assert eng.window_count(1) == 1
        exp = _check(eng, oracle_cfg, [(1, C, b"ok", 3)], [[]], state)
        assert exp[0][0] == b"[PERSON_NAME]" + b"a" * 47 + b"[PERSON_NAME]" + b"a" * 40 + b"\nok"


# ----------------------------------------------------------------------------------- dense windows
@pytest.mark.parametrize("mode", MODES)
def test_dense_windows(compiled, oracle_cfg, mode):
    """five rows of 600 bytes with a 1-byte candidate on every other byte: 1500 findings per window, past
    the window redaction kernel's LDS piece table (32 KiB slots: a row and its 300 records take 5408
    bytes, five of them do not fit the other tests' 8 KiB)"""
    from oracle import pii_oracle as O
    C = O.ROLE_CUSTOMER
    P = oracle_cfg.type_id["PERSON_NAME"]
    state = _state()
    with _engine(compiled.blob, mode, slot_bytes=32768, n_slots=8) as eng:
        for k in range(6):
            row = bytes(97 + (i + k) % 26 for i in range(600))
            exp = _check(eng, oracle_cfg, [(2, C, row, k + 1), (3, C, b"x", k + 1)],
                         [[(i, i + 1, P, 4) for i in range(0, 600, 2)], []], state)
        assert len(exp[0][1]) == 1500


# ------------------------------------------------------------------------------------- device form
def test_device_form(weng, oracle_cfg):
    """test 1's stream on other slots, its last call through pii_rescan_window_device_ext with the declared
    base and size: the host form's result.  Incremental: the enqueue relies on the declaration (a wrong one
    is found on the device and reported by the sync; nothing is read back before the launch)"""
    import torch
    E = pkg("engine")
    calls, _ = _streamed_reference()
    base = 2000
    for rows, ext, _ in calls[:-1]:
        rows = _shift(rows, base)
        weng.rescan_window([t for _, _, t, _ in rows], [c for c, _, _, _ in rows], [r for _, r, _, _ in rows],
                           [s for _, _, _, s in rows], ext=ext)
    rows, ext, exp = calls[-1]
    rows = _shift(rows, base)
    dev = torch.device("cuda", 0)
    data, offs = E.pack([t for _, _, t, _ in rows])
    n, nb = len(rows), int(offs[-1])
    spans, counts, stride = E.ext_arrays(ext, n)
    out_cap, span_cap = 5 * (nb + 48 * n) + 64, 5 * (nb // 3 + n) + 16
    d_text = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).to(dev)
    d_offs = torch.from_numpy(offs.view(np.int64).copy()).to(dev)
    d_slot = torch.tensor([c for c, _, _, _ in rows], dtype=torch.int32, device=dev)
    d_role = torch.tensor([x for _, x, _, _ in rows], dtype=torch.uint8, device=dev)
    d_ts = torch.tensor([s for _, _, _, s in rows], dtype=torch.int64, device=dev)
    d_ext = torch.from_numpy(spans.view(np.uint8).copy()).to(dev)
    d_ext_n = torch.from_numpy(counts.view(np.int32).copy()).to(dev)
    d_out = torch.zeros(out_cap + 16, dtype=torch.uint8, device=dev)
    d_oo = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_sp = torch.zeros(span_cap * 16, dtype=torch.uint8, device=dev)
    d_ctx = torch.zeros(n, dtype=torch.int16, device=dev)
    torch.cuda.synchronize(dev)
    args = lambda size: (d_text.data_ptr(), d_offs.data_ptr(), n, 0, size, d_slot.data_ptr(), d_role.data_ptr(),  # noqa
                         d_ts.data_ptr(), d_out.data_ptr(), out_cap, d_oo.data_ptr(), d_sp.data_ptr(), span_cap,
                         d_ctx.data_ptr(), d_ext.data_ptr(), d_ext_n.data_ptr(), stride)
    if weng.mode != "full":
        counts_before = [weng.window_count(c) for c, _, _, _ in rows[:3]]
        weng.rescan_window_device_ext(*args(nb - 3))                 # enqueued on the declaration alone
        with pytest.raises(E.PiiError) as ei:
            weng.sync()
        assert ei.value.code == E.PII_E_ARG
        assert [weng.window_count(c) for c, _, _, _ in rows[:3]] == counts_before
    weng.rescan_window_device_ext(*args(nb))
    ob, ns, fl = weng.sync()
    assert fl == 0

    class _R:
        out_offsets = d_oo.cpu().numpy().view(np.uint64)
        out = d_out.cpu().numpy()[:ob]
        spans = d_sp.cpu().numpy()[:ns * 16].view(E.SPAN_DTYPE)
        ctx_info = d_ctx.cpu().numpy()

        def text(self, i):
            return self.out[int(self.out_offsets[i]):int(self.out_offsets[i + 1])].tobytes()
    _compare(_R(), exp, oracle_cfg, rows)


# ------------------------------------------------------------------------------------- MASK config
def test_mask_config_takes_the_full_rescan(tmp_path, oracle_cfg):
    """a character_mask_config for PERSON_NAME: the window mode is full on its own, and every window is the
    mask applied to the helper's findings"""
    from oracle import pii_oracle as O
    E, comp = pkg("engine"), pkg("compiler")
    prim, _ = X.KNOWN_EXT[0]
    cfg = X.with_block([{"info_types": [{"name": "PERSON_NAME"}], "primitive_transformation": prim},
                        {"primitive_transformation": {"replace_with_info_type_config": {}}}])
    eng = E.Engine(comp.compile_default(X.write(tmp_path, "winext", cfg)).blob, device=0, n_conv_slots=64)
    try:
        eng.window_enable(5, 8192)
        assert eng.window_mode() == "full"
        P = eng.type_names.index("PERSON_NAME")
        assert eng.type_transform(P) == E.PII_XF_MASK
        per = _stream(oracle_cfg, seed=67, n_conv=12, per_conv=8)
        per[1][0] = ((1, O.ROLE_CUSTOMER, X.EXT_TEXT, per[1][0][0][3]), [(X.EXT_SPAN[0], X.EXT_SPAN[1], P, 4)])
        state = _state()
        masked = 0
        for k in range(8):
            rows = [per[c][k][0] for c in sorted(per)]
            ext = [per[c][k][1] for c in sorted(per)]
            res = eng.rescan_window([t for _, _, t, _ in rows], [c for c, _, _, _ in rows], [r for _, r, _, _ in rows],
                                    [s for _, _, _, s in rows], ext=ext)
            exp = WR.process_window_rows_ext(rows, ext, oracle_cfg, n=5, store=state[0], history=state[1])
            for i, (_, fs, _) in enumerate(exp):
                joined = b"\n".join(t for t, _ in state[1][rows[i][0]])
                assert res.text(i) == xform_ref.apply_transform(joined, fs, oracle_cfg.type_names, cfg), (k, i)
                assert _spans_of(res, i) == [(f.start, f.end, f.type_id, f.likelihood) for f in fs], (k, i)
                masked += any(f.type_id == P for f in fs)
            if k == 0:
                assert res.text(0) == X.KNOWN_EXT[0][1]
        assert masked > 20
    finally:
        eng.close()


# ----------------------------------------------------------------------------------------- service
def test_service_archives_no_name_in_clear(oracle_cfg):
    """PiiService with a detector: the utterance the realtime path answers with [PERSON_NAME] is archived
    with [PERSON_NAME] too, in every window that holds the row"""
    from oracle import pii_oracle as O
    from test_service import Clock
    S = pkg("service")
    ner = StubNer()
    svc = S.PiiService(n_slots=64, clock=Clock(), time_base="payload", ner=ner)
    P = oracle_cfg.type_id["PERSON_NAME"]
    texts = ["hello, who am I speaking with?", "my name is Jane Doe", "what is your email address?",
             "jane.doe@example.com", "thanks", "anything else?", "no", "bye"]
    rows = [{"conversation_id": "n1", "participant_role": "AGENT" if k % 2 == 0 else "END_USER", "text": t,
             "start_timestamp_usec": 1_000_000 * (k + 1)} for k, t in enumerate(texts)]
    body, code = svc.handle_customer_utterance({"conversation_id": "rt", "transcript": texts[1]})
    assert code == 200 and body["redacted_transcript"] == "my name is [PERSON_NAME]"
    o_rows = [("n1", O.ROLE_AGENT if k % 2 == 0 else O.ROLE_CUSTOMER, t.encode(), 1_000_000 * (k + 1))
              for k, t in enumerate(texts)]
    exp = [r.decode() for r, _, _ in WR.process_window_rows_ext(
        o_rows, ner.ext_candidates([t.encode() for t in texts], P), oracle_cfg, n=5)]
    got = [svc.rescan_window_batch([r])[0] for r in rows]
    assert got == exp
    for k, w in enumerate(got):
        assert ("my name is [PERSON_NAME]" in w.split("\n")) == (1 <= k <= 5), (k, w)
        assert "Jane Doe" not in w
    svc.engine.close()
