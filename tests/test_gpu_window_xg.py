"""The incremental window re-scan under general and text exclusion rules (PII_WINDOW_XG) on the GPU.

An engine enabled with the flag (window_mode() == "incremental", exclusion_mode() == 1) must give, window for
window, what the references give -- the oracle on "\\n".join(window), text_excl_ref.Ref for the text rules,
window_ext_ref where rows carry external candidates -- and what a second engine on the same rules gives in the
FULL re-scan: bytes, out_offsets, spans, likelihoods.  Needs an MI355X: pytest -m gpu."""
import random

import numpy as np
import pytest

import excl_configs as XC
import excl_rows as XR
import text_excl_configs as TC
import text_excl_ref as TR
import text_excl_rows as TRW
import window_ext_ref as WR
import window_xg_configs as WC
import xform_ref
from conftest import pkg

pytestmark = pytest.mark.gpu

MAKERS = {"G1": XC.g1, "G2": XC.g2, "G3": XC.g3, "plain": XC.g1_no_rules, "hx": WC.hotword_excluder,
          "nl": WC.newline_detector, "hand": TC.hand, "all_forms": TC.all_forms, "text_only": TC.text_only,
          "context": TC.context_cfg}


@pytest.fixture(scope="module")
def cfgs(tmp_path_factory):
    """name -> (config dict, compiled rules, the oracle's view of it)"""
    d = tmp_path_factory.mktemp("winxg")
    out = {}

    def get(name):
        if name not in out:
            out[name] = WC.load(d, name, MAKERS[name]())
        return out[name]
    return get


class _Eng:
    """an engine with its window enabled, closed on exit"""

    def __init__(self, blob, n=5, slot_bytes=8192, n_slots=256, **kw):
        self.e = pkg("engine").Engine(blob, device=0, n_conv_slots=n_slots)
        try:
            self.e.window_enable(n, slot_bytes, **kw)
        except Exception:
            self.e.close()
            raise

    def __enter__(self):
        return self.e

    def __exit__(self, *a):
        self.e.close()


def _pair(blob, xf=False, **kw):
    """(the flagged engine, the FULL engine) on one rule set"""
    a = _Eng(blob, incremental_exclusions=True, incremental_transforms=xf, **kw)
    try:
        b = _Eng(blob, full=True, **kw)
    except Exception:
        a.e.close()
        raise
    assert a.e.window_mode() == "incremental" and a.e.exclusion_mode() == 1
    assert b.e.window_mode() == "full"
    return a, b


def _call(eng, rows, ext=None):
    args = ([r[2] for r in rows], [r[0] for r in rows], [r[1] for r in rows], [r[3] for r in rows])
    return eng.rescan_window(*args) if ext is None else eng.rescan_window(*args, ext=ext)


def _spans(res):
    return [(int(s["utt"]), int(s["start"]), int(s["end"]), int(s["info_type"]), int(s["likelihood"]))
            for s in res.spans]


def _same(a, b, n):
    """two engines' results of one call: bytes, offsets, spans, window context"""
    assert bytes(a.out) == bytes(b.out)
    assert [int(x) for x in a.out_offsets] == [int(x) for x in b.out_offsets]
    assert _spans(a) == _spans(b)
    assert [int(x) for x in a.ctx_info[:n]] == [int(x) for x in b.ctx_info[:n]]


def _check(res, exp, rows, want=None):
    """one call's result against the reference's [(redacted window, findings, ...)]"""
    want = want if want is not None else [x[0] for x in exp]
    for i, w in enumerate(want):
        assert res.text(i) == w, (i, rows[i], res.text(i)[:160], w[:160])
    assert [int(o) for o in res.out_offsets] == [0] + [int(x) for x in np.cumsum([len(w) for w in want])]
    assert _spans(res) == [(i, f.start, f.end, f.type_id, f.likelihood) for i, x in enumerate(exp) for f in x[1]]


def _both(blob, rows, exp, want=None, ext=None, xf=False, **kw):
    """the rows in one call on the flagged engine and on the FULL engine, both against the reference"""
    a, b = _pair(blob, xf=xf, **kw)
    with a as ea, b as eb:
        ra, rb = _call(ea, rows, ext), _call(eb, rows, ext)
        _check(ra, exp, rows, want)
        _same(ra, rb, len(rows))
    return ra


# ------------------------------------------------------------------------------------------ 1 modes
def test_modes(cfgs, compiled):
    E = pkg("engine")
    eng = E.Engine(cfgs("G1")[1].blob, device=0, n_conv_slots=16)
    try:
        assert eng.exclusion_mode() == 1
        eng.window_enable(5, 4096)
        assert eng.window_mode() == "full"
        eng.window_enable(5, 4096, incremental_exclusions=True)
        assert eng.window_mode() == "incremental"        # (fails before PII_WINDOW_XG: the flag was PII_E_ARG)
        eng.window_enable(5, 4096, full=True, incremental_exclusions=True)
        assert eng.window_mode() == "full"
        eng.window_enable(5, 4096, incremental_transforms=True, incremental_exclusions=True)
        assert eng.window_mode() == "incremental"
        assert eng.lib.pii_window_enable_ex(eng.h, 5, 4096, 8) == E.PII_E_ARG
        assert eng.lib.pii_window_enable_ex(eng.h, 5, 4096, 4) == E.PII_E_ARG       # (pinned by test_gpu_window_xf.py)
        assert eng.lib.pii_window_enable_ex(eng.h, 5, 4096, E.PII_WINDOW_XG | 8) == E.PII_E_ARG
        assert eng.window_mode() == "incremental"        # a refused call leaves the window as it was
    finally:
        eng.close()
    with _Eng(compiled.blob, n_slots=16, incremental_exclusions=True) as eng:
        assert eng.window_mode() == "incremental" and eng.exclusion_mode() == 0
    with _Eng(cfgs("nl")[1].blob, n_slots=16, incremental_exclusions=True) as eng:
        assert eng.window_mode() == "full" and eng.exclusion_mode() == 1
    for name in ("G2", "hand", "text_only"):
        with _Eng(cfgs(name)[1].blob, n_slots=16, incremental_exclusions=True) as eng:
            assert eng.window_mode() == "incremental" and eng.exclusion_mode() == 1, name
        with _Eng(cfgs(name)[1].blob, n_slots=16) as eng:
            assert eng.window_mode() == "full", name
    # G3 keeps its allow-list types: it needs both flags
    with _Eng(cfgs("G3")[1].blob, n_slots=16, incremental_exclusions=True) as eng:
        assert eng.window_mode() == "full"
    with _Eng(cfgs("G3")[1].blob, n_slots=16, incremental_exclusions=True, incremental_transforms=True) as eng:
        assert eng.window_mode() == "incremental"


# ----------------------------------------------------------------------- 2 G1 and G2 over 1600 windows
@pytest.fixture(scope="module")
def g_rows():
    return WC.g_rows()


@pytest.fixture(scope="module")
def g_plain(cfgs, g_rows):
    """the oracle's windows under G1 without its rule sets: what the rules are measured against"""
    from oracle import pii_oracle as O
    return O.process_window_rows(g_rows, cfgs("plain")[2], n=5)


@pytest.mark.parametrize("name, least", [("G1", 1200), ("G2", 1)])
def test_general_rules_over_1600_windows(name, least, cfgs, g_rows, g_plain):
    from oracle import pii_oracle as O
    _, c, ocfg = cfgs(name)
    rows = g_rows
    assert len(rows) == 1600 and max(len(r[2]) for r in rows) <= 500
    exp = O.process_window_rows(rows, ocfg, n=5)
    differ = sum(1 for a, b in zip(exp, g_plain) if a[0] != b[0])
    print(name, "windows that differ from the rule-less config's:", differ)
    assert differ >= least, differ                       # the rules matter in these rows (reference alone)
    if name == "G1":
        assert exp[1][0] == b"hello\njane[OUR_DOMAIN]" and exp[3][0].endswith(b"\n[US_SOCIAL_SECURITY_NUMBER] #212-555-0187")
    _both(c.blob, rows, exp)
    if name == "G2":      # an excluder on its victim's exact span: same start, same end
        r = random.Random(3)
        texts = [t(r).encode() for _ in range(20) for t in (XR.t_domain_alone, XR.t_test_card)]
        hand = [(i // 8, O.ROLE_CUSTOMER, t, 1 + i % 8) for i, t in enumerate(texts)]
        exp = O.process_window_rows(hand, ocfg, n=5)
        base = O.process_window_rows(hand, cfgs("plain")[2], n=5)
        assert sum(1 for a, b in zip(exp, base) if a[0] != b[0]) >= 20
        _both(c.blob, hand, exp)


# ------------------------------------------------------------------- 3 the excluder's hotword across a join
@pytest.mark.parametrize("n", [5, 2])
def test_hotword_excluder_across_the_join(n, cfgs):
    from oracle import pii_oracle as O
    _, c, ocfg = cfgs("hx")
    rows = WC.hx_rows()
    exp = O.process_window_rows(rows, ocfg, n=n)
    res = _both(c.blob, rows, exp, n=n)
    if n == 5:
        for i, (red, span, lik) in WC.HX_WINDOWS.items():
            assert res.text(i) == red
            assert [(s, e, l) for u, s, e, _, l in _spans(res) if u == i] == [(span[0], span[1], lik)]
    else:                  # the hotword row has left the window: the phone number is back
        assert res.text(1) == WC.HX_WINDOWS[1][0]
        assert res.text(2) == b"4321 #[PHONE_NUMBER] ok\nx"
    # the same rows one per call: the decision is taken per window, not at arrival
    a, b = _pair(c.blob, n=n)
    with a as ea, b as eb:
        for i, r in enumerate(rows):
            ra = _call(ea, [r])
            _check(ra, [exp[i]], [r])
            _same(ra, _call(eb, [r]), 1)


# ------------------------------------------------------------------------------------------ 4 context
def test_context_changes_between_windows(cfgs):
    """the agent names a context group between two customer rows: the resident rows are decided again under the
    window's variant -- an account number passes min_likelihood only under its own context group, where the
    text rule then drops the test accounts; the phone rule holds in every variant"""
    from oracle import pii_oracle as O
    _, c, ocfg = cfgs("context")
    A, C = O.ROLE_AGENT, O.ROLE_CUSTOMER
    rows = [(0, C, b"acct 12345678901 and 00001234567", 1_000_000), (0, C, b"fax 212-555-0187 tel 212-555-0188", 2_000_000),
            (0, A, b"what is your account number", 3_000_000), (0, C, b"it is 98765432101 or 00009876543", 4_000_000),
            (1, C, b"acct 12345678901 and 00001234567", 1_000_000), (1, C, b"ok", 2_000_000)]
    exp = TR.Ref(ocfg).process_window_rows(rows, n=5)
    F = "FINANCIAL_ACCOUNT_NUMBER"
    assert [x[2] for x in exp] == [None, None, F, F, None, None]
    # the same resident row in consecutive windows: untouched without the context, decided under it
    assert exp[1][0] == b"acct 12345678901 and 00001234567\nfax 212-555-0187 tel [PHONE_NUMBER]"
    assert exp[2][0] == (b"acct [FINANCIAL_ACCOUNT_NUMBER] and 00001234567\nfax 212-555-0187 tel [PHONE_NUMBER]"
                         b"\nwhat is your account number")
    assert exp[3][0].endswith(b"\nit is [FINANCIAL_ACCOUNT_NUMBER] or 00009876543")
    _both(c.blob, rows, exp, n_slots=16)
    a, b = _pair(c.blob, n_slots=16)
    with a as ea, b as eb:
        for i, r in enumerate(rows):
            ra = _call(ea, [r])
            _check(ra, [exp[i]], [r])
            _same(ra, _call(eb, [r]), 1)


# --------------------------------------------------------------------------------------- 5 text rules
def test_text_rules_hotword_windows_across_joins(cfgs):
    _, c, ocfg = cfgs("hand")
    rows = TRW.window_convs()
    exp = TR.Ref(ocfg).process_window_rows(rows, n=5)
    assert exp[1][0] == b"this is a sample\nTK12345 is mine" and exp[4][0].endswith(b"BG1234\nvoid")
    _both(c.blob, rows, exp, n_slots=16)
    a, b = _pair(c.blob, n_slots=16)
    with a as ea, b as eb:
        for i, r in enumerate(rows):                    # every window from the ring
            ra = _call(ea, [r])
            _check(ra, [exp[i]], [r])
            _same(ra, _call(eb, [r]), 1)


@pytest.mark.parametrize("name", ["all_forms", "text_only"])
def test_text_rules_random_rows(name, cfgs):
    """text_only: no exclude_info_types list, so the marking pass is not launched"""
    from oracle import pii_oracle as O
    _, c, ocfg = cfgs(name)
    bank = pkg("synth").build_bank(0, 300, seed=31).texts
    rows = [(i // 5, O.ROLE_CUSTOMER, t, 1 + i % 5) for i, t in enumerate(bank[:300])]
    assert len(rows) == 300 and len({r[0] for r in rows}) == 60
    ref = TR.Ref(ocfg)
    exp, fired = [], set()
    store, hist = O.ContextStore(), {}
    for r in rows:
        win = hist.setdefault(r[0], [])
        win.append(r[2])
        del win[:-5]
        red, fs = ref.redact(b"\n".join(win), None)
        fired |= ref.fired
        exp.append((red, fs, None))
    assert fired, "the text rules drop candidates in these rows"
    print(name, "forms that dropped a candidate:", sorted(fired))
    _both(c.blob, rows, exp, n_slots=64)


# -------------------------------------------------------------------------------------------- 6 G3
def test_allow_list_with_kept_types_needs_both_flags(cfgs, g_rows):
    from oracle import pii_oracle as O
    cfg, c, ocfg = cfgs("G3")
    rows = g_rows[:400]
    exp = O.process_window_rows(rows, ocfg, n=5)
    hist, want = {}, []
    for r, x in zip(rows, exp):
        win = hist.setdefault(r[0], [])
        win.append(r[2])
        del win[:-5]
        want.append(xform_ref.apply_transform(b"\n".join(win), x[1], ocfg.type_names, cfg))
    assert want[1] == b"hello\njane@acme.com" and want[6].endswith(b"\n[EMAIL_ADDRESS]")
    _both(c.blob, rows, exp, want=want, xf=True)


# ------------------------------------------------------------------------------ 7 external candidates
def test_external_candidates(cfgs, g_rows):
    from oracle import pii_oracle as O
    _, c, ocfg = cfgs("G1")
    P = ocfg.type_id["PERSON_NAME"]
    rows = [(s, role, b"Ann Lee " + t, ts) for s, role, t, ts in g_rows[:320]]
    ext = [[(0, 7, P, 4)] for _ in rows]
    exp = WR.process_window_rows_ext(rows, ext, ocfg, n=5)
    assert exp[1][0] == b"[PERSON_NAME] hello\n[PERSON_NAME] jane[OUR_DOMAIN]"
    _both(c.blob, rows, exp, ext=ext)
    # rings built by plain calls, then a call that carries candidates
    a, b = _pair(c.blob)
    with a as ea, b as eb:
        state = (O.ContextStore(), {})
        for lo, hi, x in ((0, 16, False), (16, 40, True), (40, 48, False)):
            part, pe = rows[lo:hi], ext[lo:hi] if x else [[] for _ in range(lo, hi)]
            want = WR.process_window_rows_ext(part, pe, ocfg, n=5, store=state[0], history=state[1])
            ra = _call(ea, part, pe if x else None)
            _check(ra, want, part)
            _same(ra, _call(eb, part, pe if x else None), len(part))


# ---------------------------------------------------------------------------- 8 ring / batch equivalence
@pytest.mark.parametrize("slot_bytes", [8192, 640])
def test_ring_and_batch_give_the_same_windows(slot_bytes, cfgs, g_rows):
    """a window's entries come from the ring, from the batch, or from both: one row per call, all in one call,
    3 + 5 + 8 -- and with a slot so small that the arena wraps (the 16 entries take 1056 bytes with their
    candidates; 640 hold any five of them, placed in turn)"""
    from oracle import pii_oracle as O
    _, c, ocfg = cfgs("G1")
    conv = [(0, r[1], r[2], 1 + i) for i, r in enumerate(g_rows[:8] + g_rows[:8])]      # the hand rows, twice
    exp = O.process_window_rows(conv, ocfg, n=5)

    def run(splits):
        with _Eng(c.blob, slot_bytes=slot_bytes, n_slots=16, incremental_exclusions=True) as eng:
            assert eng.window_mode() == "incremental"
            out, sp = [], []
            for part in splits:
                res = _call(eng, part)
                out += [res.text(i) for i in range(len(part))]
                base = len(sp)
                sp += [[] for _ in part]
                for u, s, e, t, l in _spans(res):
                    sp[base + u].append((s, e, t, l))
            return out, sp
    one = run([[r] for r in conv])
    assert one == run([conv]) == run([conv[:3], conv[3:8], conv[8:]])
    assert one[0] == [x[0] for x in exp]
    assert one[1] == [[(f.start, f.end, f.type_id, f.likelihood) for f in x[1]] for x in exp]


# ------------------------------------------------------------------------- 9 many candidates in one entry
def test_many_candidates_in_one_entry(cfgs):
    """one 4 KB row of PAIR3 matches and SSNs: the occurrence scan's early exit, and a window whose pieces
    overflow k_win_redact's tile"""
    from oracle import pii_oracle as O
    _, c, ocfg = cfgs("G1")
    unit = b"111 222 536-22-1234 , 333 536-22-1234 ; "       # PAIR3 beside an SSN, PAIR3 over an SSN's head
    long_row = unit * 100
    assert 3900 <= len(long_row) <= 4100
    C = O.ROLE_CUSTOMER
    rows = [(0, C, b"hello 536-22-1234", 1), (0, C, long_row, 2), (0, C, b"333 536-22-1234 x", 3), (1, C, long_row, 1)]
    exp = O.process_window_rows(rows, ocfg, n=2)
    names = ocfg.type_names
    kinds = [names[f.type_id] for f in exp[1][1]]
    assert kinds.count("PAIR3") >= 150 and kinds.count("US_SOCIAL_SECURITY_NUMBER") >= 100 and len(kinds) >= 300
    assert exp[2][0].endswith(b"\n[PAIR3]-22-1234 x")
    _both(c.blob, rows, exp, n=2, slot_bytes=65536, n_slots=16)
    a, b = _pair(c.blob, n=2, slot_bytes=65536, n_slots=16)
    with a as ea, b as eb:
        for i, r in enumerate(rows):                    # the long entry read from the ring
            ra = _call(ea, [r])
            _check(ra, [exp[i]], [r])
            _same(ra, _call(eb, [r]), 1)


# ------------------------------------------------------------------------------------------ 10 growth
def test_findings_arena_and_candidate_bytes_grow_together(cfgs, g_rows):
    """a first call with one row and no candidate, then 2000 candidate-bearing rows through the device entry
    point: more window candidates than the arena's first sizing, so pii_sync grows it and runs the call again"""
    import torch
    from oracle import pii_oracle as O
    E = pkg("engine")
    _, c, ocfg = cfgs("G1")
    C = O.ROLE_CUSTOMER
    unit = b"a@acme.com 111 536-22-1234 #212-555-0187 "
    rows = [(1 + i // 8, C, unit * 3 + str(i).encode(), 1 + i % 8) for i in range(2000)]
    hist, exp = {}, []
    for r in rows:                                       # (windows repeat up to the row's number: redact once each)
        win = hist.setdefault(r[0], [])
        win.append(r[2])
        del win[:-5]
        j = b"\n".join(win)
        exp.append(O.redact(j, ocfg, None) + (None,))
    assert sum(len(x[1]) for x in exp) > 4 * len(rows)
    dev = torch.device("cuda", 0)
    with _Eng(c.blob, n_slots=512, incremental_exclusions=True) as eng:
        first = _call(eng, [(0, C, b"hello", 1)])
        assert first.text(0) == b"hello" and len(first.spans) == 0
        used0 = eng.scratch_bytes()
        data, offs = E.pack([r[2] for r in rows])
        n, nb = len(rows), int(offs[-1])
        out_cap, span_cap = 5 * (nb + 48 * n) + 64, 5 * (nb // 3 + n) + 16
        d_text = torch.from_numpy(np.concatenate([data, np.zeros(16, np.uint8)])).to(dev)
        d_offs = torch.from_numpy(offs.view(np.int64).copy()).to(dev)
        d_slot = torch.tensor([r[0] for r in rows], dtype=torch.int32, device=dev)
        d_role = torch.tensor([r[1] for r in rows], dtype=torch.uint8, device=dev)
        d_ts = torch.tensor([r[3] for r in rows], dtype=torch.int64, device=dev)
        d_out = torch.full((out_cap + 16,), 0xEE, dtype=torch.uint8, device=dev)
        d_oo = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_sp = torch.zeros(span_cap * 16, dtype=torch.uint8, device=dev)
        d_ctx = torch.zeros(n, dtype=torch.int16, device=dev)
        torch.cuda.synchronize(dev)
        eng.rescan_window_device_ex(d_text.data_ptr(), d_offs.data_ptr(), n, 0, nb, d_slot.data_ptr(),
                                    d_role.data_ptr(), d_ts.data_ptr(), d_out.data_ptr(), out_cap,
                                    d_oo.data_ptr(), d_sp.data_ptr(), span_cap, d_ctx.data_ptr())
        ob, ns, fl = eng.sync()
        assert fl == 0
        assert eng.stats(gate=True)["reruns"] >= 1               # the arena's first sizing (4 per row) was too small
        host = d_out.cpu().numpy()
        assert (host[ob:] == 0xEE).all()

        class _R:
            out_offsets = d_oo.cpu().numpy().view(np.uint64)
            out = host[:ob]
            spans = d_sp.cpu().numpy()[:ns * 16].view(E.SPAN_DTYPE)

            def text(self, i):
                return self.out[int(self.out_offsets[i]):int(self.out_offsets[i + 1])].tobytes()
        _check(_R(), exp, rows)
        assert eng.scratch_bytes() > used0
