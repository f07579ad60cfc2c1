"""pii_reidentify on the GPU: the FPE surrogates of de-identified rows decrypted in place (k_reid_check, the
deltas' scan, k_reid_pos, k_reid), given the rows and the span list the de-identify call returned.  The
reference is reid_ref (plain Python on xform_fpe_ref) over the oracle's findings; the configs are
xform_fpe_ref.F and FC, compiled as a user's config would be.  Needs an MI355X: pytest -m gpu."""
import ctypes

import numpy as np
import pytest

import reid_ref as RR
import xform_configs as X
import xform_fpe_ref as FR
import xform_ref
from conftest import pkg
from test_gpu_fpe import SWEEP, _catch_all_engine, sweep_rows

pytestmark = pytest.mark.gpu

BLOCKS = {"F": FR.F, "FC": FR.FC, "shipped": None}
# (input row, de-identified under F, re-identified; None = the input row)
LITERALS = [
    (b"card number 4111 1111 1111 1111 ok", b"card number 9329 9759 1240 5582 ok", None),
    (b"my ssn is 536-22-1234@johnny thanks", b"my ssn is 598-59-5178 thanks", b"my ssn is 536-22-1234 thanks"),
    (b"ip address 10.20.30.40 then card 4111 1111 1111 1111 ok",
     b"ip address [IP_ADDRESS] then card 9329 9759 1240 5582 ok",
     b"ip address [IP_ADDRESS] then card 4111 1111 1111 1111 ok"),
    (b"@bob_1 wrote from 10.20.30.40 call 212-555-0187 or mail jane.doe@corp.example.org",
     b" wrote from [IP_ADDRESS] call 287-927-8221 or mail c9eE.zSZ@61uc.bMX9S9N.0Xu",
     b" wrote from [IP_ADDRESS] call 212-555-0187 or mail jane.doe@corp.example.org"),
    (b"twice 4111 1111 1111 1111 and again 4111 1111 1111 1111 in one row",
     b"twice 9329 9759 1240 5582 and again 9329 9759 1240 5582 in one row", None),
]


@pytest.fixture(scope="module")
def cfgs(tmp_path_factory):
    """name -> (config dict, compiled rules)"""
    comp = pkg("compiler")
    d = tmp_path_factory.mktemp("reid")
    out = {}
    for name, block in BLOCKS.items():
        cfg = X.with_block(block)
        out[name] = (cfg, comp.compile_default(X.write(d, name, cfg)))
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


def _deid(eng, texts, ext=None, one_slot=False):
    """rows of role OTHER (no context), each its own conversation, or all of one (more rows than slots)"""
    n = len(texts)
    return eng.scan_redact(texts, [0] * n if one_slot else list(range(n)), [2] * n, [0] * n, ext=ext)


def _texts(res, n):
    return [res.text(i) for i in range(n)]


def _span_array(rows_of_findings):
    E = pkg("engine")
    recs = [(u, f.start, f.end, f.type_id, 4, 0) for u, fs in enumerate(rows_of_findings) for f in fs]
    return np.array(recs, dtype=E.SPAN_DTYPE) if recs else np.zeros(0, dtype=E.SPAN_DTYPE)


def _reid_device(eng, texts, spans, in_place=False, batch_bytes=None, out_cap=None):
    """pii_reidentify_device over uploaded rows: (status, output bytes, the 16 bytes before and after the output,
    the input buffer afterwards).  Out of place the output lies in a buffer filled with 0xEE."""
    import torch
    E = pkg("engine")
    dev = torch.device("cuda:0")
    data, offs = E.pack(texts)
    total = int(offs[-1])
    d_in = torch.from_numpy(np.concatenate([np.full(16, 0xEE, np.uint8), data, np.full(16, 0xEE, np.uint8)])).to(dev)
    d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
    raw = np.frombuffer(np.ascontiguousarray(spans, dtype=E.SPAN_DTYPE).tobytes() + bytes(16), dtype=np.uint8)
    d_sp = torch.from_numpy(raw.copy()).to(dev)
    d_out = d_in if in_place else torch.full((total + 32,), 0xEE, dtype=torch.uint8, device=dev)
    d_status = torch.full((1,), 0x7777, dtype=torch.int32, device=dev)
    eng.reidentify_device(d_in.data_ptr() + 16, d_offs.data_ptr(), len(texts), 0, total if batch_bytes is None else batch_bytes,
                          d_sp.data_ptr(), len(spans), d_out.data_ptr() + 16, total if out_cap is None else out_cap,
                          d_status.data_ptr())
    torch.cuda.synchronize()
    host, src = d_out.cpu().numpy(), d_in.cpu().numpy()
    return (int(d_status.cpu()[0]), host[16:16 + total].tobytes(), (host[:16].tobytes(), host[16 + total:].tobytes()),
            src[16:16 + total].tobytes())


# ------------------------------------------------------------------------------------------ 1 literals
def test_literals_under_F(cfgs, engines, oracle_cfg, tmp_path):
    from oracle import pii_oracle as O
    eng, cfg = engines("F"), cfgs["F"][0]
    names = oracle_cfg.type_names
    rows = [r for r, _, _ in LITERALS]
    res = _deid(eng, rows)
    assert _texts(res, len(rows)) == [d for _, d, _ in LITERALS]
    want = [r if b is None else b for r, _, b in LITERALS]
    assert eng.reidentify(_texts(res, len(rows)), res.spans) == want
    # the reference's de-identified bytes and the oracle's findings: the GPU decrypt against the Python cipher
    fs = [O.find_pii(r, oracle_cfg) for r in rows]
    de_ref = [FR.apply_transform(r, f, names, cfg) for r, f in zip(rows, fs)]
    assert eng.reidentify(de_ref, _span_array(fs)) == want == [RR.reidentify(d, f, names, cfg) for d, f in zip(de_ref, fs)]
    # a slice of whole rows, utt renumbered by the caller
    part = res.spans[res.spans["utt"] >= 2].copy()
    part["utt"] -= 2
    assert eng.reidentify(_texts(res, len(rows))[2:], part) == want[2:]
    # a1b as an external PERSON_NAME under a NUMERIC catch-all: one numeral, its "***" stays "***"
    one, _ = _catch_all_engine(tmp_path, FR.KA, "NUMERIC")
    try:
        pn = one.type_names.index("PERSON_NAME")
        r1 = _deid(one, [b"x a1b y", b"x 4111 y"], ext=[[(2, 5, pn, 4)], [(2, 6, pn, 4)]])
        assert r1.text(0) == b"x *** y" and r1.text(1) == b"x " + FR.surrogate(FR.KA, "0123456789", b"4111") + b" y"
        assert one.reidentify([r1.text(0), r1.text(1)], r1.spans) == [b"x *** y", b"x 4111 y"]
    finally:
        one.close()


# --------------------------------------------------------------------------------------- 2 length sweep
@pytest.mark.parametrize("name", list(SWEEP))
def test_length_sweep_round_trip(name, tmp_path):
    """every numeral count 0 .. nmax + 2 at all 16 residues of the packed offset.  The round trip is the input
    exactly when nmin <= n <= nmax.  Otherwise the finding became stars, and the stars stay -- except where the
    stars are themselves a numeral string of the alphabet in range (the 95-character alphabet holds '*'; n = 0
    and 1 leave 2 to 4 stars), which the decrypt form decrypts like any other: reid_ref.decrypt_piece states it."""
    E = pkg("engine")
    common, custom = SWEEP[name]
    alphabet = custom or FR.COMMON[common]
    eng, cfg = _catch_all_engine(tmp_path, FR.KC, common, custom, person_only=True)
    try:
        pn = eng.type_names.index("PERSON_NAME")
        texts, ext, counts = sweep_rows(alphabet, pn)
        nmin, nmax = FR.limits(len(alphabet))
        res = _deid(eng, texts, ext=ext)
        assert len(res.spans) == len(texts)
        back = eng.reidentify(_texts(res, len(texts)), res.spans)
        star_runs = 0
        for i, (t, xs) in enumerate(zip(texts, ext)):
            s, e = xs[0][:2]
            in_range = nmin <= counts[i] <= nmax
            assert (back[i] == t) == in_range, (i, counts[i])
            if not in_range:
                stars = b"*" * (e - s)
                assert res.text(i) == t[:s] + stars + t[e:]
                assert back[i] == t[:s] + RR.decrypt_piece(FR.KC, alphabet, stars) + t[e:]
                if "*" not in alphabet or FR.fallen_back(alphabet, stars):
                    assert back[i] == res.text(i)
                    star_runs += 1
        assert star_runs >= 2 * 16          # at least the counts above nmax
        if "*" not in alphabet:
            assert star_runs == (nmin + 2) * 16
    finally:
        eng.close()


# ------------------------------------------------------------------------------- 3 corpus, device calls
@pytest.fixture(scope="module")
def corpus(oracle_cfg):
    from oracle import pii_oracle as O
    synth = pkg("synth")
    bank = synth.build_bank(600, 600, seed=7)
    corp = synth.make_corpus(263, 37, bank, seed=3)          # 9731 rows, context variants live
    rows = [(int(corp.conv_slot[i]), int(corp.role[i]),
             corp.data[int(corp.offsets[i]):int(corp.offsets[i + 1])].tobytes(), int(corp.ts_us[i]))
            for i in range(corp.n)]
    return corp, rows, O.process_rows(rows, oracle_cfg)


@pytest.mark.parametrize("name", ["F", "FC"])
def test_corpus_scan_then_reidentify_on_one_stream(name, cfgs, corpus, oracle_cfg):
    """scan_redact_device, reidentify_device out of place and reidentify_device in place, enqueued back to back:
    the second and third read the spans and the offsets the first wrote, no host round trip in between.  The sizes
    the calls are told (output bytes, span count) come from the reference."""
    import torch
    corp, rows, exp = corpus
    assert corp.n == 9731
    cfg, names = cfgs[name][0], oracle_cfg.type_names
    E = pkg("engine")
    de = [FR.apply_transform(r[2], x[1], names, cfg) for r, x in zip(rows, exp)]
    want = [RR.reidentify(d, x[1], names, cfg) for d, x in zip(de, exp)]
    ob, ns = sum(len(d) for d in de), sum(len(x[1]) for x in exp)
    fell = encrypted = 0
    for r, x in zip(rows, exp):
        for f in x[1]:
            fpe = FR.fpe_of(xform_ref.pick(names[f.type_id], cfg))
            if fpe is not None:
                encrypted += 1
                fell += FR.fallen_back(FR.alphabet_of(fpe), r[2][f.start:f.end])
    assert fell == 0 and encrypted > 0              # no finding falls back: the star rule hides no wrong cipher
    if name == "FC":
        assert encrypted == ns == 1040 and want == [r[2] for r in rows]
    dev = torch.device("cuda:0")
    n = corp.n
    d_text = torch.from_numpy(np.concatenate([corp.data, np.zeros(64, np.uint8)])).to(dev)
    d_offs = torch.from_numpy(np.ascontiguousarray(corp.offsets).view(np.int64)).to(dev)
    d_slot = torch.from_numpy(np.ascontiguousarray(corp.conv_slot, dtype=np.uint32).view(np.int32)).to(dev)
    d_role = torch.from_numpy(np.ascontiguousarray(corp.role, dtype=np.uint8)).to(dev)
    d_ts = torch.from_numpy(np.ascontiguousarray(corp.ts_us, dtype=np.int64)).to(dev)
    out_cap, span_cap = int(corp.offsets[-1]) * 2 + 64 * n, n * 4
    d_out = torch.full((out_cap + 32,), 0xEE, dtype=torch.uint8, device=dev)
    d_oo = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_sp = torch.empty(span_cap * 16, dtype=torch.uint8, device=dev)
    d_ctx = torch.empty(n, dtype=torch.int16, device=dev)
    d_re = torch.full((ob + 32,), 0xEE, dtype=torch.uint8, device=dev)
    d_status = torch.full((2,), 0x7777, dtype=torch.int32, device=dev)
    eng = E.Engine(cfgs[name][1].blob, device=0, n_conv_slots=1 << 12)         # fresh conversation contexts
    scan = lambda: eng.scan_redact_device(                                  # noqa: E731
        d_text.data_ptr(), d_offs.data_ptr(), n, d_slot.data_ptr(), d_role.data_ptr(), d_ts.data_ptr(), d_out.data_ptr(),
        out_cap, d_oo.data_ptr(), d_sp.data_ptr(), span_cap, d_ctx.data_ptr())
    try:
        # A first call sizes the work queues and opens the long-row gate: what pii_sync repairs by running a call
        # again, which a call enqueued behind it would not see.  Then the conversations' contexts are dropped, so
        # the second pass computes what a fresh engine would.
        scan()
        assert eng.sync() == (ob, ns, 0)
        for s in sorted(set(int(x) for x in corp.conv_slot)):
            eng.context_set(s, -1, 0)
        d_out.fill_(0xEE)
        d_oo.zero_()
        d_sp.zero_()
        torch.cuda.synchronize()
        eng.histogram_reset()
        scan()
        eng.reidentify_device(d_out.data_ptr(), d_oo.data_ptr(), n, 0, ob, d_sp.data_ptr(), ns, d_re.data_ptr() + 16, ob,
                              d_status.data_ptr())
        eng.reidentify_device(d_out.data_ptr(), d_oo.data_ptr(), n, 0, ob, d_sp.data_ptr(), ns, d_out.data_ptr(), out_cap,
                              d_status.data_ptr() + 4)
        torch.cuda.synchronize()
        # the scan call is still the one pii_sync answers for, and the histogram is the scan's
        assert eng.sync() == (ob, ns, 0) and eng.stats(gate=True)["reruns"] == 0
        hist = eng.histogram()
    finally:
        eng.close()
    assert d_status.cpu().tolist() == [0, 0]
    spans = np.frombuffer(d_sp[:ns * 16].cpu().numpy().tobytes(), dtype=E.SPAN_DTYPE)
    assert [(int(s["utt"]), int(s["start"]), int(s["end"]), int(s["info_type"])) for s in spans] == [
        (i, f.start, f.end, f.type_id) for i, x in enumerate(exp) for f in x[1]]
    assert (hist == np.bincount(spans["info_type"].astype(np.int64), minlength=len(hist))[:len(hist)]).all()
    oo = d_oo.cpu().numpy()
    assert [int(o) for o in oo] == [0] + list(np.cumsum([len(d) for d in de]))
    re_host, in_place = d_re.cpu().numpy(), d_out.cpu().numpy()
    assert re_host[:16].tobytes() == b"\xee" * 16 and re_host[16 + ob:].tobytes() == b"\xee" * 16
    assert in_place[ob:ob + 16].tobytes() == b"\xee" * 16
    for i, w in enumerate(want):
        lo, hi = int(oo[i]), int(oo[i + 1])
        assert re_host[16 + lo:16 + hi].tobytes() == w, (i, rows[i][2])
        assert in_place[lo:hi].tobytes() == w, (i, rows[i][2])


# ----------------------------------------------------------------------- 4 the prefix across a scan tile
def test_row_of_4500_spans_across_the_scan_tile(cfgs, engines, oracle_cfg):
    from oracle import pii_oracle as O
    eng, cfg = engines("F"), cfgs["F"][0]
    names = oracle_cfg.type_names
    rows = [LITERALS[0][0], LITERALS[1][0], LITERALS[3][0], b"@bob_1 a@b.co 10.20.30.40 " * 1500, LITERALS[2][0]]
    fs = [O.find_pii(r, oracle_cfg) for r in rows]
    assert [names[f.type_id] for f in fs[3][:3]] == ["SOCIAL_HANDLE", "EMAIL_ADDRESS", "IP_ADDRESS"]
    assert len(fs[3]) == 4500
    before = sum(len(f) for f in fs[:3])
    assert 0 < before < 4096 < before + 4500              # the row starts after span 0 and straddles the tile
    res = _deid(eng, rows)
    assert len(res.spans) == sum(len(f) for f in fs)
    de = _texts(res, len(rows))
    assert de == [FR.apply_transform(r, f, names, cfg) for r, f in zip(rows, fs)]
    assert de[3] == b" g@d.35 [IP_ADDRESS] " * 1500
    back = eng.reidentify(de, res.spans)
    assert back == [RR.reidentify(d, f, names, cfg) for d, f in zip(de, fs)]
    assert back[3] == b" a@b.co [IP_ADDRESS] " * 1500
    assert back[4] == LITERALS[2][2]


def test_more_spans_than_the_single_pass_scan_takes(cfgs, engines, oracle_cfg):
    """above 64 tiles of 4096 spans the deltas' prefix takes the reduce / scan-of-sums / apply kernels: 66000 copies
    of the row with a -6 and a +1 delta before its two FPE findings, between two other rows (the reference is
    computed once per distinct row)"""
    from oracle import pii_oracle as O
    eng, cfg = engines("F"), cfgs["F"][0]
    names = oracle_cfg.type_names
    distinct = [LITERALS[0][0], LITERALS[3][0], LITERALS[2][0]]
    fs = [O.find_pii(r, oracle_cfg) for r in distinct]
    de = [FR.apply_transform(r, f, names, cfg) for r, f in zip(distinct, fs)]
    want = [RR.reidentify(d, f, names, cfg) for d, f in zip(de, fs)]
    copies = 66000
    assert len(fs[1]) * copies > 64 * 4096
    res = _deid(eng, [distinct[0]] + [distinct[1]] * copies + [distinct[2]], one_slot=True)
    assert len(res.spans) == len(fs[0]) + len(fs[1]) * copies + len(fs[2])
    assert res.out.tobytes() == de[0] + de[1] * copies + de[2]
    back = eng.reidentify([de[0]] + [de[1]] * copies + [de[2]], res.spans)
    assert b"".join(back) == want[0] + want[1] * copies + want[2]
    assert back[1] == back[copies] == LITERALS[3][2] and back[-1] == LITERALS[2][2]


# ------------------------------------------------------------------------------------------ 5 bad spans
def _bad_lists(good, n_types, row_len):
    """name -> a span list with one defect; good: the spans of LITERALS[:3] (card; SSN, handle; IP, card)"""
    assert [int(u) for u in good["utt"]] == [0, 1, 1, 2, 2]
    out = {}
    s = good.copy()
    s[[1, 2]] = s[[2, 1]]
    out["swapped"] = s
    s = good.copy()
    s[2]["start"] = s[1]["end"] - 1
    out["overlap"] = s
    s = good.copy()
    s[4]["utt"] = 3
    out["utt"] = s
    s = good.copy()
    s[0]["info_type"] = n_types
    out["type"] = s
    s = good.copy()
    s[3]["end"] = s[3]["start"]
    out["empty"] = s
    s = good.copy()
    s[4]["end"] = row_len + 5
    out["end"] = s
    # well-formed and ordered, but four one-byte IP_ADDRESS findings (+11 bytes each) push the card out of row 2
    ip = int(good[3]["info_type"])
    extra = np.array([(2, k, k + 1, ip, 4, 0) for k in range(4)], dtype=good.dtype)
    s = np.concatenate([good[:3], extra, good[4:]])
    s[-1]["start"], s[-1]["end"] = 20, 39
    out["deltas"] = s
    return out


def test_bad_spans_leave_the_rows_alone(cfgs, engines):
    E = pkg("engine")
    eng = engines("F")
    rows = [r for r, _, _ in LITERALS[:3]]
    res = _deid(eng, rows)
    de = _texts(res, 3)
    want = [r if b is None else b for r, _, b in LITERALS[:3]]
    n_types = len(eng.type_names)
    bad = _bad_lists(res.spans, n_types, len(rows[2]))
    assert len(bad) == 7
    for what, spans in bad.items():
        with pytest.raises(E.PiiError) as ei:
            eng.reidentify(de, spans)
        assert ei.value.code == E.PII_E_ARG and "span" in str(ei.value), what
        for in_place in (False, True):
            status, out, guards, src = _reid_device(eng, de, spans, in_place=in_place)
            assert status == E.PII_REID_BAD_SPAN, what
            assert out == b"".join(de) and src == b"".join(de), what
            assert guards == (b"\xee" * 16, b"\xee" * 16), what
        # the next well-formed call on the same engine succeeds
        assert eng.reidentify(de, res.spans) == want, what
    status, out, guards, src = _reid_device(eng, de, res.spans)
    assert status == 0 and out == b"".join(want) and src == b"".join(de) and guards == (b"\xee" * 16, b"\xee" * 16)
    status, out, guards, _ = _reid_device(eng, de, res.spans, in_place=True)
    assert status == 0 and out == b"".join(want) and guards == (b"\xee" * 16, b"\xee" * 16)


def test_bad_arguments(engines):
    import torch
    E = pkg("engine")
    eng = engines("F")
    rows = [r for r, _, _ in LITERALS[:3]]
    res = _deid(eng, rows)
    de = _texts(res, 3)
    total = sum(len(d) for d in de)
    # a declared size that is not the offsets': detected on the device, nothing decrypted
    status, out, _, _ = _reid_device(eng, de, res.spans, batch_bytes=total - 1, out_cap=total)
    assert status == E.PII_REID_BAD_ARGS and out[:total - 1] == b"".join(de)[:total - 1]
    # a short out_cap, device and host
    with pytest.raises(E.PiiError) as ei:
        _reid_device(eng, de, res.spans, out_cap=total - 1)
    assert ei.value.code == E.PII_E_CAPACITY
    data, offs = E.pack(de)
    out = np.zeros(total, np.uint8)
    sp = np.ascontiguousarray(res.spans)
    rc = eng.lib.pii_reidentify(eng.h, data.ctypes.data_as(ctypes.c_void_p), offs.ctypes.data_as(ctypes.c_void_p), 3,
                                sp.ctypes.data_as(ctypes.c_void_p), len(sp), out.ctypes.data_as(ctypes.c_void_p), total - 1)
    assert rc == E.PII_E_CAPACITY and not out.any()
    # an output that overlaps the rows without being the rows
    dev = torch.device("cuda:0")
    d_buf = torch.from_numpy(np.concatenate([data, np.zeros(64, np.uint8)])).to(dev)
    d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_sp = torch.from_numpy(np.frombuffer(sp.tobytes(), dtype=np.uint8).copy()).to(dev)
    d_status = torch.zeros(1, dtype=torch.int32, device=dev)
    for shift in (8, total - 1):
        with pytest.raises(E.PiiError) as ei:
            eng.reidentify_device(d_buf.data_ptr(), d_offs.data_ptr(), 3, 0, total, d_sp.data_ptr(), len(sp),
                                  d_buf.data_ptr() + shift, total, d_status.data_ptr())
        assert ei.value.code == E.PII_E_ARG
    torch.cuda.synchronize()
    assert d_buf.cpu().numpy()[:total].tobytes() == b"".join(de)
    assert eng.reidentify(de, res.spans) == [r if b is None else b for r, _, b in LITERALS[:3]]


# ----------------------------------------------------------------------------------- 6 degenerate shapes
def test_degenerate_shapes(cfgs, engines, oracle_cfg):
    E = pkg("engine")
    eng = engines("F")
    none = np.zeros(0, dtype=E.SPAN_DTYPE)
    assert eng.reidentify([], none) == []
    status, out, _, _ = _reid_device(eng, [], none)
    assert status == 0 and out == b""
    assert eng.reidentify([b"", b""], none) == [b"", b""]
    # empty rows between full ones
    rows = [b"", LITERALS[0][0], b"", b"", LITERALS[2][0], b""]
    res = _deid(eng, rows)
    back = eng.reidentify(_texts(res, len(rows)), res.spans)
    assert back == [b"", LITERALS[0][0], b"", b"", LITERALS[2][2], b""]
    for in_place in (False, True):
        status, out, _, _ = _reid_device(eng, _texts(res, len(rows)), res.spans, in_place=in_place)
        assert status == 0 and out == b"".join(back)
    # no spans: the copy
    plain = [b"nothing to find in this row", b"", b"nor in this one"]
    assert eng.reidentify(plain, none) == plain
    status, out, _, _ = _reid_device(eng, plain, none)
    assert status == 0 and out == b"".join(plain)
    # the shipped config has no FPE type: the spans are checked, the output is the copy
    shipped = engines("shipped")
    rows = [r for r, _, _ in LITERALS[:4]]
    res = _deid(shipped, rows)
    assert res.text(0) == b"card number [CREDIT_CARD_NUMBER] ok" and len(res.spans) == 9
    assert shipped.reidentify(_texts(res, 4), res.spans) == _texts(res, 4)
    status, out, _, _ = _reid_device(shipped, _texts(res, 4), res.spans)
    assert status == 0 and out == b"".join(_texts(res, 4))
    s = res.spans.copy()
    s[[0, 1]] = s[[1, 0]]
    with pytest.raises(E.PiiError):
        shipped.reidentify(_texts(res, 4), s)


# ----------------------------------------------------------------------------------- 7 window, service
def test_window_rescan_results_reidentify_as_they_are(cfgs, oracle_cfg):
    from oracle import pii_oracle as O
    E = pkg("engine")
    cfg, names = cfgs["F"][0], oracle_cfg.type_names
    conv = [(7, O.ROLE_CUSTOMER, t, 10 + k) for k, t in enumerate(
        [LITERALS[0][0], b"nothing here", LITERALS[3][0], LITERALS[1][0], b"mail a@b.co and c@d.io", LITERALS[2][0]])]
    eng = E.Engine(cfgs["F"][1].blob, device=0, n_conv_slots=64)
    try:
        eng.window_enable(5, 32768, incremental_transforms=True)
        assert eng.window_mode() == "incremental"
        store, hist, win = O.ContextStore(), {}, []
        decrypted = 0
        for batch in (conv[:2], conv[2:3], conv[3:]):
            res = eng.rescan_window([r[2] for r in batch], [r[0] for r in batch], [r[1] for r in batch],
                                    [r[3] for r in batch])
            exp = O.process_window_rows(batch, oracle_cfg, n=5, store=store, history=hist)
            back = eng.reidentify(_texts(res, len(batch)), res.spans)
            for i, (r, (_, fs, _)) in enumerate(zip(batch, exp)):
                win.append(r[2])
                del win[:-5]
                de = FR.apply_transform(b"\n".join(win), fs, names, cfg)
                assert res.text(i) == de
                assert back[i] == RR.reidentify(de, fs, names, cfg), (i, de)
                decrypted += sum(names[f.type_id] in FR.F_FPE for f in fs)
        assert len(win) == 5 and decrypted >= 15
        assert back[-1].endswith(b"\n" + LITERALS[2][2]) and b"4111 1111 1111 1111" in back[-1]
    finally:
        eng.close()


def test_service_end_to_end(cfgs):
    E, S = pkg("engine"), pkg("service")
    from test_service import Clock
    eng = E.Engine(cfgs["F"][1].blob, device=0, n_conv_slots=64)
    try:
        svc = S.PiiService(engine=eng, clock=Clock(), time_base="payload")
        rows = [{"conversation_id": f"c{i}", "participant_role": "END_USER", "text": r.decode(),
                 "start_timestamp_usec": 10 + i} for i, (r, _, _) in enumerate(LITERALS)]
        rows.append({"conversation_id": "c9", "participant_role": "END_USER", "start_timestamp_usec": 30,
                     "text": "José Núñez écrit à jane.doe@corp.example.org — merci"})
        found = []
        red = svc.process_batch(rows, findings=found)
        assert red[:len(LITERALS)] == [d.decode() for _, d, _ in LITERALS]
        assert found[1] == [{"start": 10, "end": 21, "info_type": "US_SOCIAL_SECURITY_NUMBER"},
                            {"start": 21, "end": 28, "info_type": "SOCIAL_HANDLE"}]
        back = svc.reidentify_batch([{"text": t, "findings": f} for t, f in zip(red, found)] +
                                    [{"text": "[DLP_API_CALL_ERROR] x", "findings": None}])
        assert back[:len(LITERALS)] == [(r if b is None else b).decode() for r, _, b in LITERALS]
        assert red[-1] != rows[-1]["text"] and back[-2] == rows[-1]["text"]
        assert back[-1] == "[DLP_API_CALL_ERROR] x"
        with pytest.raises(E.PiiError) as ei:
            svc.reidentify_batch([{"text": red[0], "findings": [{"start": 12, "end": 60, "info_type": "CREDIT_CARD_NUMBER"}]}])
        assert ei.value.code == E.PII_E_ARG
    finally:
        eng.close()
