"""deidentify_config on the GPU: mask / replace / remove / keep per info type, against xform_ref applied
to the oracle's findings (the oracle ignores the block, so detection stays the reference).

Configs (xform_configs): A = card / SSN / phone masks, e-mail replaced, handles removed, the rest kept;
B = one catch-all mask (every row keeps its length); C = everything removed but the masked card;
D = replace / remove only (the kinds the incremental window path keeps; only under D do the window test's
dense rows reach k_win_redact's slow path, A and B take the FULL re-scan).  Needs an MI355X: pytest -m gpu."""
import ctypes

import numpy as np
import pytest

import xform_configs as X
import xform_ref
from conftest import pkg

pytestmark = pytest.mark.gpu

D = [{"info_types": [{"name": "EMAIL_ADDRESS"}],
      "primitive_transformation": {"replace_config": {"new_value": {"string_value": "<email>"}}}},
     {"info_types": [{"name": "SOCIAL_HANDLE"}], "primitive_transformation": {"redact_config": {}}},
     {"primitive_transformation": {"replace_with_info_type_config": {}}}]
BLOCKS = {"A": X.A, "B": X.B, "C": X.C, "D": D, "shipped": None}
CARD = b"4111 1111 1111 1111"


@pytest.fixture(scope="module")
def cfgs(tmp_path_factory):
    """name -> (config dict, compiled rules), compiled from a JSON file as a user's config would be"""
    comp = pkg("compiler")
    d = tmp_path_factory.mktemp("xf")
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


def _rows(texts, role=2):
    return [(i, role, t, 0) for i, t in enumerate(texts)]


def _expect(rows, oracle_cfg, cfg, extra=None):
    from oracle import pii_oracle as O
    exp = O.process_rows(rows, oracle_cfg, extra=extra)
    return [xform_ref.apply_transform(r[2], x[1], oracle_cfg.type_names, cfg) for r, x in zip(rows, exp)], exp


def _check_host(eng, rows, oracle_cfg, cfg, ext=None):
    """host entry point: every row's bytes, the offsets, the spans and the histogram"""
    want, exp = _expect(rows, oracle_cfg, cfg, ext)
    eng.histogram_reset()
    res = eng.scan_redact([r[2] for r in rows], [r[0] for r in rows], [r[1] for r in rows], [r[3] for r in rows],
                          ext=ext)
    for i, w in enumerate(want):
        assert res.text(i) == w, (i, rows[i][2][:80], res.text(i)[:80], w[:80])
    assert [int(o) for o in res.out_offsets] == [0] + list(np.cumsum([len(w) for w in want]))
    got = [(int(s["utt"]), int(s["start"]), int(s["end"]), int(s["info_type"]), int(s["likelihood"]))
           for s in res.spans]
    assert got == [(i, f.start, f.end, f.type_id, f.likelihood) for i, x in enumerate(exp) for f in x[1]]
    hist = eng.histogram()
    assert (hist == np.bincount(res.spans["info_type"].astype(np.int64), minlength=len(hist))[:len(hist)]).all()
    return res


# ------------------------------------------------------------------------------------ 1 known answers
def test_known_answers(cfgs, engines, oracle_cfg):
    E = pkg("engine")
    eng = engines("A")
    rows = _rows([t for t, _ in X.KNOWN_A])
    res = _check_host(eng, rows, oracle_cfg, cfgs["A"][0])
    for i, (_, want) in enumerate(X.KNOWN_A):
        assert res.text(i) == want
    kinds = {"CREDIT_CARD_NUMBER": E.PII_XF_MASK, "US_SOCIAL_SECURITY_NUMBER": E.PII_XF_MASK,
             "PHONE_NUMBER": E.PII_XF_MASK, "EMAIL_ADDRESS": E.PII_XF_REPLACE, "SOCIAL_HANDLE": E.PII_XF_REDACT}
    for t, name in enumerate(eng.type_names):
        assert eng.type_transform(t) == kinds.get(name, E.PII_XF_KEEP), name
    with pytest.raises(E.PiiError):
        eng.type_transform(len(eng.type_names))
    shipped = engines("shipped")
    assert {shipped.type_transform(t) for t in range(len(shipped.type_names))} == {E.PII_XF_INFO_TYPE}


@pytest.mark.parametrize("k", range(len(X.KNOWN_EXT)))
def test_known_answers_external_candidate(k, tmp_path, oracle_cfg):
    E, comp = pkg("engine"), pkg("compiler")
    prim, want = X.KNOWN_EXT[k]
    cfg = X.with_block([{"info_types": [{"name": "PERSON_NAME"}], "primitive_transformation": prim}])
    eng = E.Engine(comp.compile_default(X.write(tmp_path, "ext", cfg)).blob, device=0, n_conv_slots=16)
    try:
        pn = eng.type_names.index("PERSON_NAME")
        ext = [[(X.EXT_SPAN[0], X.EXT_SPAN[1], pn, 4)], []]
        res = _check_host(eng, _rows([X.EXT_TEXT, b"plain row"]), oracle_cfg, cfg, ext)
        assert res.text(0) == want and res.text(1) == b"plain row"
        assert eng.type_transform(pn) == E.PII_XF_MASK
    finally:
        eng.close()


@pytest.mark.parametrize("which", sorted(X.LONG_MASKS))
def test_masked_candidate_of_several_windows_at_every_alignment(which, tmp_path, oracle_cfg):
    """the mask walk past its first 16-byte window: a 68-byte external candidate of 1- to 4-byte code points
    (X.LONG_NAME; the entry point does not limit a candidate's length) whose code points straddle the
    window edges of both directions, at each of the 16 alignments of its first byte, masked whole and up to
    a count that runs out in the second (forward) or third (reverse) window"""
    E, comp = pkg("engine"), pkg("compiler")
    prim = X.LONG_MASKS[which]
    cfg = X.with_block([{"info_types": [{"name": "PERSON_NAME"}], "primitive_transformation": prim}])
    eng = E.Engine(comp.compile_default(X.write(tmp_path, "long", cfg)).blob, device=0, n_conv_slots=16)
    try:
        pn = eng.type_names.index("PERSON_NAME")
        assert eng.type_transform(pn) == E.PII_XF_MASK
        texts, spans = X.long_rows()
        _, offs = E.pack(texts)
        assert {(int(offs[i]) + s) % 16 for i, (s, _) in enumerate(spans)} == set(range(16))
        res = _check_host(eng, _rows(texts), oracle_cfg, cfg, [[(s, e, pn, 4)] for s, e in spans])
        masked = xform_ref.mask(X.LONG_NAME, prim["character_mask_config"])
        for i, (t, (s, e)) in enumerate(zip(texts, spans)):
            assert res.text(i) == t[:s] + masked + t[e:], i
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------ 2 corpus
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


def _run_device(eng, data, offsets, slot, role, ts, out_cap, span_cap, shift=0):
    """device entry point; the output pointer `shift` bytes past a 16-byte boundary"""
    import torch
    dev = torch.device("cuda:0")
    n = len(offsets) - 1
    d_text = torch.from_numpy(np.concatenate([data, np.zeros(64, np.uint8)])).to(dev)
    d_offs = torch.from_numpy(np.ascontiguousarray(offsets).view(np.int64)).to(dev)
    d_slot = torch.from_numpy(np.ascontiguousarray(slot, dtype=np.uint32).view(np.int32)).to(dev)
    d_role = torch.from_numpy(np.ascontiguousarray(role, dtype=np.uint8)).to(dev)
    d_ts = torch.from_numpy(np.ascontiguousarray(ts, dtype=np.int64)).to(dev)
    d_out = torch.zeros(out_cap + 32, dtype=torch.uint8, device=dev)
    assert d_out.data_ptr() % 16 == 0
    d_oo = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_sp = torch.empty(span_cap * 16, dtype=torch.uint8, device=dev)
    d_ctx = torch.empty(max(n, 1), dtype=torch.int16, device=dev)
    eng.histogram_reset()
    eng.scan_redact_device(d_text.data_ptr(), d_offs.data_ptr(), n, d_slot.data_ptr(), d_role.data_ptr(),
                           d_ts.data_ptr(), d_out.data_ptr() + shift, out_cap, d_oo.data_ptr(), d_sp.data_ptr(),
                           span_cap, d_ctx.data_ptr())
    ob, ns, flags = eng.sync()
    assert flags == 0
    E = pkg("engine")
    return (d_out[shift:shift + ob].cpu().numpy().tobytes(), d_oo.cpu().numpy(),
            np.frombuffer(d_sp[:ns * 16].cpu().numpy().tobytes(), dtype=E.SPAN_DTYPE), eng.histogram())


@pytest.mark.parametrize("name", ["A", "B", "C", "shipped"])
def test_corpus(name, cfgs, engines, corpus, oracle_cfg):
    corp, rows, exp = corpus
    cfg = cfgs[name][0]
    E = pkg("engine")
    eng = E.Engine(cfgs[name][1].blob, device=0, n_conv_slots=1 << 12)     # fresh conversation contexts
    try:
        out, oo, spans, hist = _run_device(eng, corp.data, corp.offsets, corp.conv_slot, corp.role, corp.ts_us,
                                           int(corp.offsets[-1]) * 2 + 64 * corp.n, corp.n * 4)
    finally:
        eng.close()
    names = oracle_cfg.type_names
    assert len(spans) == sum(len(x[1]) for x in exp)
    assert (hist == np.bincount(spans["info_type"].astype(np.int64), minlength=len(hist))[:len(hist)]).all()
    for i, (r, x) in enumerate(zip(rows, exp)):
        got = out[int(oo[i]):int(oo[i + 1])]
        assert got == xform_ref.apply_transform(r[2], x[1], names, cfg), (i, r[2])
        if name == "B":
            assert len(got) == len(r[2])
        if name == "shipped":
            assert got == x[0]                     # the default path: the oracle's own "[TYPE]" redaction
    assert int(oo[corp.n]) == len(out)


# ------------------------------------------------------------------------------- 3 block / tile edges
FILL = (b"lorem ipsum " * 5461)[:65529] + b" "                    # 65530 bytes without a finding
# The first row of each batch: FILL, then findings.  Redaction tiles are 64 KiB of output ADDRESSES, so
# with the output pointer `shift` bytes past a 16-byte boundary the first tile edge lies at batch output
# offset 65536 - shift: 65521 .. 65536.  Per (config, row): the batch OUTPUT offset and output length
# each finding must have (the row is the batch's first, so its output offsets are the batch's).
#   card:    a masked card across the edge for shifts 0..5 and starting on it at shift 6
#   mail_1st: the e-mail at output 65530 -- under C removed (zero bytes exactly on the edge at shift 6, the
#            removed handle one byte later at shift 5), under A a 7-byte replacement across the edge
#   mail_2nd: the handle removed at 65530 (A and C); the e-mail at output 65536, the edge itself at shift 0
#            (a finding that begins where the tile ends): replaced under A, removed under C
EDGE_ROWS = {"card": FILL + CARD + b" ok and more text after the edge",
             "mail_1st": FILL + b"a@b.co @johnny tail after the edge 536-22-1234 end",
             "mail_2nd": FILL + b"@johnny word a@b.co tail after the edge 536-22-1234 end"}
EDGE_WANT = {
    ("A", "card"): [("CREDIT_CARD_NUMBER", 65530, 19)], ("C", "card"): [("CREDIT_CARD_NUMBER", 65530, 19)],
    ("A", "mail_1st"): [("EMAIL_ADDRESS", 65530, 7), ("SOCIAL_HANDLE", 65538, 0),
                        ("US_SOCIAL_SECURITY_NUMBER", 65559, 11)],
    ("C", "mail_1st"): [("EMAIL_ADDRESS", 65530, 0), ("SOCIAL_HANDLE", 65531, 0),
                        ("US_SOCIAL_SECURITY_NUMBER", 65552, 0)],
    ("A", "mail_2nd"): [("SOCIAL_HANDLE", 65530, 0), ("EMAIL_ADDRESS", 65536, 7),
                        ("US_SOCIAL_SECURITY_NUMBER", 65564, 11)],
    ("C", "mail_2nd"): [("SOCIAL_HANDLE", 65530, 0), ("EMAIL_ADDRESS", 65536, 0),
                        ("US_SOCIAL_SECURITY_NUMBER", 65557, 0)],
}


@pytest.mark.parametrize("name,case", sorted(EDGE_WANT))
def test_tile_edge_at_every_output_misalignment(name, case, cfgs, engines, oracle_cfg):
    """a masked, a replaced and a removed finding whose OUTPUT lies on the first 64 KiB tile edge, at each
    of the 16 misalignments of the output pointer (which sweep the edge across the finding and onto it)"""
    eng, cfg = engines(name), cfgs[name][0]
    texts = [EDGE_ROWS[case], b"second row @johnny 10.20.30.40", b"", b"last row a@b.co"]
    rows = _rows(texts)
    want, exp = _expect(rows, oracle_cfg, cfg)
    names = oracle_cfg.type_names
    # where the reference puts each finding of the first row in the batch's output, and how many bytes
    fs, placed = exp[0][1], []
    for k, f in enumerate(fs):
        at = len(xform_ref.apply_transform(texts[0][:f.start], fs[:k], names, cfg))
        end = len(xform_ref.apply_transform(texts[0][:f.end], fs[:k + 1], names, cfg))
        placed.append((names[f.type_id], at, end - at))
    assert placed == EDGE_WANT[name, case]
    data, offs = pkg("engine").pack(texts)
    n = len(texts)
    for shift in range(16):
        out, oo, spans, _ = _run_device(eng, data, offs, np.arange(n), np.full(n, 2), np.zeros(n), len(data) + 256,
                                        64, shift)
        for i, w in enumerate(want):
            assert out[int(oo[i]):int(oo[i + 1])] == w, (shift, i)
        assert len(spans) == sum(len(x[1]) for x in exp)


# --------------------------------------------------------------- 4 more spans than one pass holds
@pytest.mark.parametrize("name", ["A", "C", "B"])
def test_more_spans_than_one_redact_pass(name, cfgs, engines, oracle_cfg):
    from oracle import pii_oracle as O
    text = b"a@b.co " * 400 + CARD
    fs = O.find_pii(text, oracle_cfg)
    # precondition: one 64 KiB output tile starts more findings than one assembly pass holds (255)
    assert len(fs) > 255 and len(text) < 65536
    _check_host(engines(name), _rows([text, b"tail row a@b.co"]), oracle_cfg, cfgs[name][0])


# ------------------------------------------------------------------------------------- 5 cut rows
@pytest.mark.parametrize("name", ["A", "C"])
def test_cut_row_with_findings_across_lane_cuts(name, cfgs, engines, oracle_cfg):
    """a small batch scans 128-byte lanes and cuts a row longer than two of them: a card number across
    byte 128, an SSN directly followed by a handle across byte 256 (length-preserving and zero-length
    outputs in the per-lane deltas k_rowlen and k_sel_fix add up)"""
    from oracle import pii_oracle as O
    pad = b"lorem ipsum dolor sit amet consectetur adipiscing elit sed do eiusmod tempor incididunt ut labore "
    row = (pad * 2)[:120] + CARD + b" "
    row += (pad * 2)[:247 - len(row)] + b" 536-22-1234@johnny "
    row += (pad * 8)[:700 - len(row)]
    assert len(row) == 700
    fs = O.find_pii(row, oracle_cfg)
    names = oracle_cfg.type_names
    assert [(f.start, f.end, names[f.type_id]) for f in fs] == [
        (120, 139, "CREDIT_CARD_NUMBER"), (248, 259, "US_SOCIAL_SECURITY_NUMBER"), (259, 266, "SOCIAL_HANDLE")]
    eng = engines(name)
    _check_host(eng, _rows([b"short row", row, b"mail a@b.co"]), oracle_cfg, cfgs[name][0])
    assert eng.stats()["lane_bytes"] == 128


# ---------------------------------------------------------------------------------- 6 empty results
def test_every_row_becomes_empty(cfgs, engines, oracle_cfg):
    texts = [b"@johnny", b"@bob_1", b"@TechieTom", b"@a_b_c_9"] * 16
    res = _check_host(engines("A"), _rows(texts), oracle_cfg, cfgs["A"][0])
    assert len(res.out) == 0 and not res.out_offsets.any() and len(res.spans) == len(texts)


def test_empty_rows_rows_that_become_empty_and_untouched_rows(cfgs, engines, oracle_cfg):
    texts = [b"", b"@johnny", b"no finding here", b"", b"@bob_1", b"ip address 10.20.30.40", b"@johnny", b""] * 8
    for name in ("A", "C"):
        _check_host(engines(name), _rows(texts), oracle_cfg, cfgs[name][0])


# ------------------------------------------------------------------------------------- 7 capacity
def test_capacity_reports_the_transformed_size_and_commits_nothing(cfgs, engines, oracle_cfg):
    from oracle import pii_oracle as O
    E = pkg("engine")
    eng, cfg = engines("A"), cfgs["A"][0]
    agent = b"What is your email address?"
    assert O.extract_expected_pii(agent, oracle_cfg)
    slot = 77
    rows = [(slot, O.ROLE_AGENT, agent, 1), (slot, O.ROLE_CUSTOMER, b"it is jane.doe@corp.example.org @johnny", 2),
            (slot, O.ROLE_CUSTOMER, b"card " + CARD + b" and 212-555-0187", 3)]
    want, exp = _expect(rows, oracle_cfg, cfg)
    need, nsp = sum(len(w) for w in want), sum(len(x[1]) for x in exp)
    assert need != sum(len(r[2]) for r in rows)
    assert eng.context_get(slot)[0] == -1
    data, offs = E.pack([r[2] for r in rows])
    n = len(rows)
    sl, rl = np.full(n, slot, np.uint32), np.array([r[1] for r in rows], np.uint8)
    ts = np.array([r[3] for r in rows], np.int64)

    def call(out_cap):
        out, oo = np.zeros(need + 64, np.uint8), np.zeros(n + 1, np.uint64)
        spans, ns, ctx = np.zeros(64, E.SPAN_DTYPE), ctypes.c_uint32(0), np.zeros(n, np.int16)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)          # noqa: E731
        rc = eng.lib.pii_scan_redact(eng.h, p(data), p(offs), n, p(sl), p(rl), p(ts), p(out), out_cap, p(oo),
                                     p(spans), 64, ctypes.byref(ns), p(ctx))
        return rc, out, oo, ns.value

    rc, out, oo, ns = call(need - 1)
    assert rc == E.PII_E_CAPACITY
    assert (int(oo[n]), ns) == (need, nsp)
    assert eng.context_get(slot)[0] == -1                 # the AGENT row's context was not committed
    rc, out, oo, ns = call(need)
    assert rc == E.PII_OK and (int(oo[n]), ns) == (need, nsp)
    assert out[:need].tobytes() == b"".join(want)
    assert eng.group_types[eng.context_get(slot)[0]] == exp[0][3]


# --------------------------------------------------------------------------------------- 8 window
WINDOW_MODE = {"A": "full", "B": "full", "D": "incremental"}     # mask / keep kinds re-scan in full


@pytest.mark.parametrize("name", ["A", "B", "D"])
def test_window_rescan(name, cfgs, oracle_cfg):
    from oracle import pii_oracle as O
    E, synth = pkg("engine"), pkg("synth")
    cfg = cfgs[name][0]
    bank = synth.build_bank(400, 900, seed=41)
    corp = synth.make_corpus(40, 12, bank, seed=42)
    rows = [(int(corp.conv_slot[i]), int(corp.role[i]),
             corp.data[int(corp.offsets[i]):int(corp.offsets[i + 1])].tobytes(), int(corp.ts_us[i]))
            for i in range(corp.n)]
    # a conversation whose windows hold more pieces than the window kernel's LDS table (its slow path)
    dense = [(3000, O.ROLE_CUSTOMER, b"a@b.co " * 120, 10 + k) for k in range(6)]
    eng = E.Engine(cfgs[name][1].blob, device=0, n_conv_slots=4096)
    try:
        eng.window_enable(5, 32768)
        assert eng.window_mode() == WINDOW_MODE[name]
        store, hist, mine = O.ContextStore(), {}, {}
        names = oracle_cfg.type_names
        for batch in (rows[:len(rows) // 2], rows[len(rows) // 2:] + dense[:2], dense[2:]):
            res = eng.rescan_window([r[2] for r in batch], [r[0] for r in batch], [r[1] for r in batch],
                                    [r[3] for r in batch])
            exp = O.process_window_rows(batch, oracle_cfg, n=5, store=store, history=hist)
            for i, (r, (_, fs, _)) in enumerate(zip(batch, exp)):
                win = mine.setdefault(r[0], [])
                win.append(r[2])
                del win[:-5]
                assert res.text(i) == xform_ref.apply_transform(b"\n".join(win), fs, names, cfg), (i, r)
                m = res.spans["utt"] == i
                assert [(int(s["start"]), int(s["end"]), int(s["info_type"])) for s in res.spans[m]] == [
                    (f.start, f.end, f.type_id) for f in fs]
    finally:
        eng.close()
