"""crypto_hash_config on the GPU: findings replaced by base64(HMAC-SHA256(key, finding bytes)), against
xform_hash_ref (hmac / hashlib) applied to the oracle's findings; the oracle ignores deidentify_config, so
detection stays the reference.

Configs (xform_hash_ref): H = card, SSN and e-mail hashed under key 1, phone under key 2, handles removed,
the rest "[TYPE]"; HC = one catch-all hash under key 1.  Needs an MI355X: pytest -m gpu."""
import ctypes

import numpy as np
import pytest

import xform_configs as X
import xform_hash_ref as HR
from blob_damage import (_hash_key_dropped, _hash_mid_dropped, _key_index_out_of_range, _key_table_short,
                         _mid_cut_short, _placeholder_short)
from conftest import pkg

pytestmark = pytest.mark.gpu

BLOCKS = {"H": HR.H, "HC": HR.HC, "shipped": None}
CARD = HR.CARD
KNOWN_TEXTS = [b"card number 4111 1111 1111 1111 ok",
               b"my ssn is 536-22-1234@johnny thanks",
               b"twice 4111 1111 1111 1111 and again 4111 1111 1111 1111 in one row",
               b"call 212-555-0187 or mail jane.doe@corp.example.org",
               b"another conversation: 4111 1111 1111 1111",
               b"ip address 10.20.30.40 and @bob_1"]


@pytest.fixture(scope="module")
def cfgs(tmp_path_factory):
    """name -> (config dict, compiled rules), compiled from a JSON file as a user's config would be"""
    comp = pkg("compiler")
    d = tmp_path_factory.mktemp("xfh")
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
    return [HR.apply_transform(r[2], x[1], oracle_cfg.type_names, cfg) for r, x in zip(rows, exp)], exp


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


def _run_device(eng, data, offsets, slot, role, ts, out_cap, span_cap, shift=0):
    """device entry point; the output pointer `shift` bytes past a 16-byte boundary.  The output buffer is
    filled with 0xEE: (bytes, offsets, spans, histogram, what lies before and after the output)"""
    import torch
    dev = torch.device("cuda:0")
    n = len(offsets) - 1
    d_text = torch.from_numpy(np.concatenate([data, np.zeros(64, np.uint8)])).to(dev)
    d_offs = torch.from_numpy(np.ascontiguousarray(offsets).view(np.int64)).to(dev)
    d_slot = torch.from_numpy(np.ascontiguousarray(slot, dtype=np.uint32).view(np.int32)).to(dev)
    d_role = torch.from_numpy(np.ascontiguousarray(role, dtype=np.uint8)).to(dev)
    d_ts = torch.from_numpy(np.ascontiguousarray(ts, dtype=np.int64)).to(dev)
    d_out = torch.full((out_cap + 32,), 0xEE, dtype=torch.uint8, device=dev)
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
    host = d_out.cpu().numpy()
    return (host[shift:shift + ob].tobytes(), d_oo.cpu().numpy(),
            np.frombuffer(d_sp[:ns * 16].cpu().numpy().tobytes(), dtype=E.SPAN_DTYPE), eng.histogram(),
            (host[:shift].tobytes(), host[shift + ob:shift + ob + 16].tobytes()))


# ------------------------------------------------------------------------------------ 1 known answers
def test_known_answers(cfgs, engines, oracle_cfg):
    from oracle import pii_oracle as O
    E = pkg("engine")
    eng = engines("H")
    names = oracle_cfg.type_names
    fs = O.find_pii(KNOWN_TEXTS[0], oracle_cfg)
    assert [(f.start, f.end, names[f.type_id]) for f in fs] == [(12, 31, "CREDIT_CARD_NUMBER")]
    fs = O.find_pii(KNOWN_TEXTS[1], oracle_cfg)
    assert [(f.start, f.end, names[f.type_id]) for f in fs] == [(10, 21, "US_SOCIAL_SECURITY_NUMBER"),
                                                                 (21, 28, "SOCIAL_HANDLE")]
    res = _check_host(eng, _rows(KNOWN_TEXTS), oracle_cfg, cfgs["H"][0])
    assert res.text(0) == b"card number " + HR.CARD_KEY1 + b" ok"
    assert res.text(1) == b"my ssn is " + HR.SSN_KEY1 + b" thanks"      # a hash directly followed by a removed finding
    # the same card: the same surrogate, twice in one row and in another conversation
    assert res.text(2) == b"twice " + HR.CARD_KEY1 + b" and again " + HR.CARD_KEY1 + b" in one row"
    assert res.text(4) == b"another conversation: " + HR.CARD_KEY1
    # the phone is hashed under key 2, the e-mail under key 1
    phone, mail = b"212-555-0187", b"jane.doe@corp.example.org"
    assert res.text(3) == b"call " + HR.surrogate(HR.KEY2, phone) + b" or mail " + HR.surrogate(HR.KEY1, mail)
    assert res.text(5) == b"ip address [IP_ADDRESS] and "
    # under HC the same digits are hashed under key 1: the phone's surrogate differs, the card's does not
    res_c = _check_host(engines("HC"), _rows(KNOWN_TEXTS), oracle_cfg, cfgs["HC"][0])
    assert res_c.text(0) == res.text(0)
    assert res_c.text(3).startswith(b"call " + HR.surrogate(HR.KEY1, phone) + b" or mail ")
    assert res_c.text(3)[5:49] != res.text(3)[5:49] and res_c.text(3)[49:] == res.text(3)[49:]
    kinds = {n: E.PII_XF_HASH for n in HR.H_HASHED}
    kinds["SOCIAL_HANDLE"] = E.PII_XF_REDACT
    for t, name in enumerate(eng.type_names):
        assert eng.type_transform(t) == kinds.get(name, E.PII_XF_INFO_TYPE), name
    hc = engines("HC")
    assert {hc.type_transform(t) for t in range(len(hc.type_names))} == {E.PII_XF_HASH} and E.PII_XF_HASH == 5


# ------------------------------------------------------------ 2 padding boundaries and input alignment
PAD_LENGTHS = (1, 55, 56, 63, 64, 65, 119, 120, 127, 128, 1000)
LOREM = (b"lorem ipsum dolor sit amet consectetur adipiscing elit sed do eiusmod tempor incididunt ut labore et "
         b"dolore magna aliqua ut enim ad minim veniam quis nostrud exercitation ullamco laboris nisi ut aliquip ")


def test_padding_boundaries_at_every_input_alignment(tmp_path, oracle_cfg):
    """external PERSON_NAME candidates over filler text: every span length around SHA-256's padding
    boundaries (len % 64 = 55 / 56, one and two blocks, a long one), each starting at 16 consecutive byte
    offsets of the packed batch (every row is a multiple of 16 bytes long)"""
    E, comp = pkg("engine"), pkg("compiler")
    cfg = X.with_block([{"info_types": [{"name": "PERSON_NAME"}], "primitive_transformation": HR.hash_prim(HR.KEY1)},
                        {"primitive_transformation": {"replace_with_info_type_config": {}}}])
    eng = E.Engine(comp.compile_default(X.write(tmp_path, "pad", cfg)).blob, device=0, n_conv_slots=1 << 10)
    try:
        pn = eng.type_names.index("PERSON_NAME")
        assert eng.type_transform(pn) == E.PII_XF_HASH
        fill = LOREM * 8
        texts, ext, starts = [], [], {}
        for li, n in enumerate(PAD_LENGTHS):
            for j in range(16):
                size = (j + n + 15) // 16 * 16
                rot = (li * 16 + j) * 7 % len(LOREM)
                texts.append(fill[rot:rot + size])
                ext.append([(j, j + n, pn, 4)])
        texts.append(X.EXT_TEXT)
        ext.append([(X.EXT_SPAN[0], X.EXT_SPAN[1], pn, 4)])
        _, offs = E.pack(texts)
        for i, xs in enumerate(ext[:-1]):
            starts.setdefault(xs[0][1] - xs[0][0], set()).add((int(offs[i]) + xs[0][0]) % 16)
        assert starts == {n: set(range(16)) for n in PAD_LENGTHS}
        res = _check_host(eng, _rows(texts), oracle_cfg, cfg, ext)
        assert len(res.spans) == len(texts)
        for i, (t, xs) in enumerate(zip(texts, ext)):
            s, e = xs[0][:2]
            assert res.text(i) == t[:s] + HR.surrogate(HR.KEY1, t[s:e]) + t[e:]
        assert res.text(len(texts) - 1) == b"I am " + HR.JOSE_KEY1 + b" ok"
    finally:
        eng.close()


# ------------------------------------------------------------------------------- 3 output tile edge
FILL = (b"lorem ipsum " * 5461)[:65529] + b" "                    # 65530 bytes without a finding


def test_surrogate_across_the_tile_edge_at_every_output_misalignment(cfgs, engines, oracle_cfg):
    """redaction tiles are 64 KiB of output addresses: with the output pointer `shift` bytes past a 16-byte
    boundary the first tile edge lies at batch output 65536 - shift: inside the 44 bytes that start at 65530
    for shifts 0..5, where they start at shift 6, up to 9 bytes before them at the larger shifts"""
    eng, cfg = engines("H"), cfgs["H"][0]
    texts = [FILL + CARD + b" ok and more text after the edge", b"second row @johnny 10.20.30.40", b"",
             b"last row a@b.co"]
    rows = _rows(texts)
    want, exp = _expect(rows, oracle_cfg, cfg)
    names = oracle_cfg.type_names
    assert [(names[f.type_id], f.start, f.end) for f in exp[0][1]] == [("CREDIT_CARD_NUMBER", 65530, 65549)]
    assert want[0][65530:65574] == HR.CARD_KEY1 and want[0][:65530] == FILL
    data, offs = pkg("engine").pack(texts)
    n = len(texts)
    for shift in range(16):
        assert (65530 < 65536 - shift < 65530 + 44) == (shift < 6)
        out, oo, spans, _, (before, after) = _run_device(eng, data, offs, np.arange(n), np.full(n, 2), np.zeros(n),
                                                         len(data) + 256, 64, shift)
        for i, w in enumerate(want):
            assert out[int(oo[i]):int(oo[i + 1])] == w, (shift, i)
        assert len(spans) == sum(len(x[1]) for x in exp)
        assert before == b"\xee" * shift and after == b"\xee" * 16       # nothing outside the output


# ------------------------------------------------------------------------------------------ 4 corpus
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


@pytest.mark.parametrize("name", ["H", "HC"])
def test_corpus(name, cfgs, corpus, oracle_cfg):
    corp, rows, exp = corpus
    assert corp.n == 9731
    cfg = cfgs[name][0]
    E = pkg("engine")
    eng = E.Engine(cfgs[name][1].blob, device=0, n_conv_slots=1 << 12)     # fresh conversation contexts
    try:
        out, oo, spans, hist, _ = _run_device(eng, corp.data, corp.offsets, corp.conv_slot, corp.role, corp.ts_us,
                                              int(corp.offsets[-1]) * 2 + 64 * corp.n, corp.n * 4)
    finally:
        eng.close()
    names = oracle_cfg.type_names
    assert len(spans) == sum(len(x[1]) for x in exp)
    assert (hist == np.bincount(spans["info_type"].astype(np.int64), minlength=len(hist))[:len(hist)]).all()
    got_spans = [(int(s["utt"]), int(s["start"]), int(s["end"]), int(s["info_type"])) for s in spans]
    assert got_spans == [(i, f.start, f.end, f.type_id) for i, x in enumerate(exp) for f in x[1]]
    for i, (r, x) in enumerate(zip(rows, exp)):
        got = out[int(oo[i]):int(oo[i + 1])]
        assert got == HR.apply_transform(r[2], x[1], names, cfg), (i, r[2])
        if name == "HC":
            assert len(got) == len(r[2]) + sum(44 - (f.end - f.start) for f in x[1])
    assert int(oo[corp.n]) == len(out)
    assert HR.PLACEHOLDER not in out


# ------------------------------------------------------------------------------------- 5 cut rows
def test_cut_row_with_findings_across_lane_cuts(cfgs, engines, oracle_cfg):
    """a small batch scans 128-byte lanes and cuts a row longer than two of them: a card number across
    byte 128, an SSN directly followed by a handle across byte 256 (the fixed 44-byte and the zero-length
    outputs in the per-lane deltas add up)"""
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
    eng = engines("H")
    res = _check_host(eng, _rows([b"short row", row, b"mail a@b.co"]), oracle_cfg, cfgs["H"][0])
    assert eng.stats()["lane_bytes"] == 128
    assert res.text(1) == row[:120] + HR.CARD_KEY1 + row[139:248] + HR.SSN_KEY1 + row[266:]


# ------------------------------------------------------------------------------------- 6 capacity
def test_capacity_reports_the_transformed_size_and_commits_nothing(cfgs, engines, oracle_cfg):
    from oracle import pii_oracle as O
    E = pkg("engine")
    eng, cfg = engines("H"), cfgs["H"][0]
    agent = b"What is your email address?"
    assert O.extract_expected_pii(agent, oracle_cfg)
    slot = 77
    rows = [(slot, O.ROLE_AGENT, agent, 1), (slot, O.ROLE_CUSTOMER, b"it is jane.doe@corp.example.org @johnny", 2),
            (slot, O.ROLE_CUSTOMER, b"card " + CARD + b" and 212-555-0187", 3)]
    want, exp = _expect(rows, oracle_cfg, cfg)
    need, nsp = sum(len(w) for w in want), sum(len(x[1]) for x in exp)
    size_in = sum(len(r[2]) for r in rows)
    assert need > size_in                                 # the hashed output is longer than the input
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

    rc, out, oo, ns = call(size_in)                       # a capacity sized for the input
    assert rc == E.PII_E_CAPACITY
    assert (int(oo[n]), ns) == (need, nsp)
    assert eng.context_get(slot)[0] == -1                 # the AGENT row's context was not committed
    rc, out, oo, ns = call(need)
    assert rc == E.PII_OK and (int(oo[n]), ns) == (need, nsp)
    assert out[:need].tobytes() == b"".join(want)
    assert eng.group_types[eng.context_get(slot)[0]] == exp[0][3]


# --------------------------------------------------------------------------------------- 7 window
def test_window_rescan_takes_the_full_path(cfgs, oracle_cfg):
    from oracle import pii_oracle as O
    E, synth = pkg("engine"), pkg("synth")
    cfg = cfgs["H"][0]
    bank = synth.build_bank(400, 900, seed=41)
    corp = synth.make_corpus(40, 12, bank, seed=42)
    rows = [(int(corp.conv_slot[i]), int(corp.role[i]),
             corp.data[int(corp.offsets[i]):int(corp.offsets[i + 1])].tobytes(), int(corp.ts_us[i]))
            for i in range(corp.n)]
    # a conversation of e-mail addresses only: windows of several hundred surrogates, 7 times their input
    dense = [(3000, O.ROLE_CUSTOMER, b"a@b.co " * 120, 10 + k) for k in range(6)]
    eng = E.Engine(cfgs["H"][1].blob, device=0, n_conv_slots=4096)
    try:
        eng.window_enable(5, 32768)
        assert eng.window_mode() == "full"
        store, hist, mine = O.ContextStore(), {}, {}
        names = oracle_cfg.type_names
        hashed = 0
        for batch in (rows[:len(rows) // 2], rows[len(rows) // 2:] + dense[:2], dense[2:]):
            res = eng.rescan_window([r[2] for r in batch], [r[0] for r in batch], [r[1] for r in batch],
                                    [r[3] for r in batch])
            exp = O.process_window_rows(batch, oracle_cfg, n=5, store=store, history=hist)
            for i, (r, (_, fs, _)) in enumerate(zip(batch, exp)):
                win = mine.setdefault(r[0], [])
                win.append(r[2])
                del win[:-5]
                assert res.text(i) == HR.apply_transform(b"\n".join(win), fs, names, cfg), (i, r)
                assert HR.PLACEHOLDER not in res.text(i)
                m = res.spans["utt"] == i
                assert [(int(s["start"]), int(s["end"]), int(s["info_type"])) for s in res.spans[m]] == [
                    (f.start, f.end, f.type_id) for f in fs]
                hashed += sum(names[f.type_id] in HR.H_HASHED for f in fs)
        assert hashed >= 120 * (1 + 2 + 3 + 4 + 5 + 5)    # the dense conversation's windows alone
    finally:
        eng.close()


# -------------------------------------------------------------------------------- 8 malformed blobs
@pytest.mark.parametrize("damage", [_hash_mid_dropped, _hash_key_dropped, _key_index_out_of_range, _mid_cut_short,
                                    _key_table_short, _placeholder_short], ids=lambda f: f.__name__.strip("_"))
def test_malformed_hash_sections_are_rejected(damage, cfgs):
    import inspect
    E, comp = pkg("engine"), pkg("compiler")
    c = cfgs["H"][1]
    S = comp.blob_sections(c.blob)
    assert comp._sections_to_blob(S) == c.blob              # the round trip itself changes nothing
    if len(inspect.signature(damage).parameters) == 2:
        damage(S, c.rules.type_names)
    else:
        damage(S)
    with pytest.raises(E.PiiError):
        E.Engine(comp._sections_to_blob(S), device=0, n_conv_slots=16).close()


# --------------------------------------------------------------------------------- 9 default path
def test_shipped_config_still_gives_the_type_tokens(cfgs, engines, oracle_cfg):
    rows = _rows(KNOWN_TEXTS)
    res = _check_host(engines("shipped"), rows, oracle_cfg, cfgs["shipped"][0])
    _, exp = _expect(rows, oracle_cfg, cfgs["shipped"][0])
    for i, x in enumerate(exp):
        assert res.text(i) == x[0]                          # the oracle's own "[TYPE]" redaction
    assert res.text(0) == b"card number [CREDIT_CARD_NUMBER] ok"
