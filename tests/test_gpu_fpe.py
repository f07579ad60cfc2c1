"""crypto_replace_ffx_fpe_config on the GPU: a finding's characters of the alphabet encrypted among themselves
with FF1 over AES (k_fpe, k_win_fpe), against xform_fpe_ref (plain Python) applied to the oracle's findings;
the oracle ignores deidentify_config, so detection stays the reference.  Spans, offsets and the histogram
are compared with the oracle throughout.

Configs (xform_fpe_ref): F = card, SSN and phone NUMERIC under KA, SWIFT and IBAN UPPER_CASE_ALPHA_NUMERIC under
KC, e-mail ALPHA_NUMERIC under KB, handles removed, the rest "[TYPE]"; FC = one catch-all ALPHA_NUMERIC under
KA.  Needs an MI355X: pytest -m gpu."""
import base64
import random

import numpy as np
import pytest

import fpe_damage as FD
import xform_configs as X
import xform_fpe_ref as FR
import xform_hash_ref
from conftest import pkg

pytestmark = pytest.mark.gpu

BLOCKS = {"F": FR.F, "FC": FR.FC, "shipped": None}
CARD = FR.CARD
KNOWN_TEXTS = [b"card number 4111 1111 1111 1111 ok",
               b"my ssn is 536-22-1234@johnny thanks",
               b"twice 4111 1111 1111 1111 and again 4111 1111 1111 1111 in one row",
               b"call 212-555-0187 or mail jane.doe@corp.example.org",
               b"another conversation: 4111 1111 1111 1111",
               b"ip address 10.20.30.40 and @bob_1"]
LOREM = (b"lorem ipsum dolor sit amet consectetur adipiscing elit sed do eiusmod tempor incididunt ut labore et "
         b"dolore magna aliqua ut enim ad minim veniam quis nostrud exercitation ullamco laboris nisi ut aliquip ")


@pytest.fixture(scope="module")
def cfgs(tmp_path_factory):
    """name -> (config dict, compiled rules), compiled from a JSON file as a user's config would be"""
    comp = pkg("compiler")
    d = tmp_path_factory.mktemp("xff")
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


def _catch_all_engine(tmp_path, key, common=None, custom=None, person_only=False):
    """(engine, config) of one FPE transformation: for every type, or for PERSON_NAME with "[TYPE]" for the rest"""
    E, comp = pkg("engine"), pkg("compiler")
    prim = FR.fpe_prim(key, common, custom)
    block = [{"primitive_transformation": prim}]
    if person_only:
        block = [{"info_types": [{"name": "PERSON_NAME"}], "primitive_transformation": prim},
                 {"primitive_transformation": {"replace_with_info_type_config": {}}}]
    cfg = X.with_block(block)
    return E.Engine(comp.compile_default(X.write(tmp_path, "one", cfg)).blob, device=0, n_conv_slots=1 << 12), cfg


def _rows(texts, role=2):
    return [(i, role, t, 0) for i, t in enumerate(texts)]


def _expect(rows, oracle_cfg, cfg, extra=None):
    from oracle import pii_oracle as O
    exp = O.process_rows(rows, oracle_cfg, extra=extra)
    return [FR.apply_transform(r[2], x[1], oracle_cfg.type_names, cfg) for r, x in zip(rows, exp)], exp


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
    eng = engines("F")
    names = oracle_cfg.type_names
    fs = O.find_pii(KNOWN_TEXTS[0], oracle_cfg)
    assert [(f.start, f.end, names[f.type_id]) for f in fs] == [(12, 31, "CREDIT_CARD_NUMBER")]
    fs = O.find_pii(KNOWN_TEXTS[1], oracle_cfg)
    assert [(f.start, f.end, names[f.type_id]) for f in fs] == [(10, 21, "US_SOCIAL_SECURITY_NUMBER"),
                                                                 (21, 28, "SOCIAL_HANDLE")]
    res = _check_host(eng, _rows(KNOWN_TEXTS), oracle_cfg, cfgs["F"][0])
    assert res.text(0) == b"card number 9329 9759 1240 5582 ok"
    assert res.text(1) == b"my ssn is 598-59-5178 thanks"          # an FPE finding directly followed by a removed one
    # the same card: the same surrogate, twice in one row and in another conversation
    assert res.text(2) == b"twice 9329 9759 1240 5582 and again 9329 9759 1240 5582 in one row"
    assert res.text(4) == b"another conversation: 9329 9759 1240 5582"
    # the phone under NUMERIC and KA, the e-mail under ALPHA_NUMERIC and KB
    mail = FR.surrogate(FR.KB, FR.COMMON["ALPHA_NUMERIC"], b"jane.doe@corp.example.org")
    assert res.text(3) == b"call " + FR.surrogate(FR.KA, "0123456789", b"212-555-0187") + b" or mail " + mail
    assert res.text(5) == b"ip address [IP_ADDRESS] and "
    kinds = {n: E.PII_XF_FPE for n in FR.F_FPE}
    kinds["SOCIAL_HANDLE"] = E.PII_XF_REDACT
    for t, name in enumerate(eng.type_names):
        assert eng.type_transform(t) == kinds.get(name, E.PII_XF_INFO_TYPE), name
    fc = engines("FC")
    assert {fc.type_transform(t) for t in range(len(fc.type_names))} == {E.PII_XF_FPE} and E.PII_XF_FPE == 6
    # under FC the same rows keep their lengths; the e-mail is the literal of ALPHA_NUMERIC under KA
    res_c = _check_host(fc, _rows(KNOWN_TEXTS), oracle_cfg, cfgs["FC"][0])
    assert [len(res_c.text(i)) for i in range(len(KNOWN_TEXTS))] == [len(t) for t in KNOWN_TEXTS]
    assert res_c.text(3).endswith(b" or mail 29mg.NbJ@hdTC.vACRK0X.wtl")


# one engine per (alphabet, key): a catch-all, so whichever type the finding gets is encrypted with it; the
# finding is also given as an external PERSON_NAME candidate, for the literals no detector finds
LITERALS = {}
for _p, _a, _k, _w in FR.KNOWN:
    LITERALS.setdefault((_a, _k), []).append((_p, _w))
for _k, _w in FR.NIST_EMPTY.items():
    LITERALS.setdefault(("NUMERIC", _k), []).append((FR.NIST_DIGITS, _w))


@pytest.mark.parametrize("combo", list(LITERALS), ids=lambda c: "%s_%d_%02x" % (c[0], len(c[1]), c[1][0]))
def test_literals(combo, tmp_path, oracle_cfg):
    """the issue's table and the three empty-tweak NIST samples: each finding alone in a row, between "x " and " y" """
    alphabet, key = combo
    eng, cfg = _catch_all_engine(tmp_path, key, alphabet)
    try:
        pn = eng.type_names.index("PERSON_NAME")
        texts = [b"x " + p + b" y" for p, _ in LITERALS[combo]]
        ext = [[(2, 2 + len(p), pn, 4)] for p, _ in LITERALS[combo]]
        res = _check_host(eng, _rows(texts), oracle_cfg, cfg, ext)
        for i, (p, w) in enumerate(LITERALS[combo]):
            assert res.text(i) == b"x " + w + b" y", (p, res.text(i))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------ 2 length sweep
SEPARATORS = ["·".encode(), "é".encode(), "€".encode()]             # outside every alphabet, 2 and 3 bytes
SWEEP = {"NUMERIC": ("NUMERIC", None), "ALPHA_NUMERIC": ("ALPHA_NUMERIC", None), "custom95": (None, FR.ALPHA95)}


def sweep_rows(alphabet: str, pn: int):
    """every numeral count 0 .. nmax + 2, each starting at 16 consecutive offsets of the packed batch (every row
    is a multiple of 16 bytes long); a separator follows every numeral, so no detector fires inside"""
    _, nmax = FR.limits(len(alphabet))
    rnd = random.Random(len(alphabet))
    fill = LOREM * 4
    texts, ext, counts = [], [], []
    for n in range(nmax + 3):
        numerals = b"".join(rnd.choice(alphabet).encode() + SEPARATORS[(n + k) % 3] for k in range(n))
        for j in range(16):
            piece = numerals or SEPARATORS[j % 3]
            size = (j + len(piece) + 1 + 15) // 16 * 16
            rot = (n * 16 + j) * 7 % len(LOREM)
            texts.append(fill[rot:rot + j] + piece + b" " + fill[rot + j:rot + size - len(piece) - 1])
            ext.append([(j, j + len(piece), pn, 4)])
            counts.append(n)
    return texts, ext, counts


@pytest.mark.parametrize("name", list(SWEEP))
def test_length_sweep_at_every_input_alignment(name, tmp_path, oracle_cfg):
    E = pkg("engine")
    common, custom = SWEEP[name]
    alphabet = custom or FR.COMMON[common]
    eng, cfg = _catch_all_engine(tmp_path, FR.KC, common, custom, person_only=True)
    try:
        pn = eng.type_names.index("PERSON_NAME")
        assert eng.type_transform(pn) == E.PII_XF_FPE
        texts, ext, counts = sweep_rows(alphabet, pn)
        _, offs = E.pack(texts)
        starts = {}
        for i, xs in enumerate(ext):
            starts.setdefault(counts[i], set()).add((int(offs[i]) + xs[0][0]) % 16)
        nmin, nmax = FR.limits(len(alphabet))
        assert starts == {n: set(range(16)) for n in range(nmax + 3)}
        res = _check_host(eng, _rows(texts), oracle_cfg, cfg, ext)
        assert len(res.spans) == len(texts)                      # the candidate alone, in every row
        for i, (t, xs) in enumerate(zip(texts, ext)):
            s, e = xs[0][:2]
            assert e - s > counts[i] or counts[i] == 0           # separators: the finding is longer than n
            got = res.text(i)
            assert got == t[:s] + FR.surrogate(FR.KC, alphabet, t[s:e]) + t[e:]
            assert (got[s:e] == b"*" * (e - s)) == (not nmin <= counts[i] <= nmax)
    finally:
        eng.close()


# ------------------------------------------------------------------------------- 3 output tile edge
FILL = (b"lorem ipsum " * 5461)[:65518] + b" "                    # 65519 bytes without a finding


def test_card_across_the_tile_edge_at_every_output_misalignment(cfgs, engines, oracle_cfg):
    """redaction tiles are 64 KiB of output addresses: with the output pointer `shift` bytes past a 16-byte
    boundary the first tile edge lies at batch output 65536 - shift, inside the card's 19 bytes from 65519 at
    every shift"""
    eng, cfg = engines("F"), cfgs["F"][0]
    texts = [FILL + CARD + b" ok and more text after the edge", b"second row @johnny 10.20.30.40", b"",
             b"last row a@b.co"]
    rows = _rows(texts)
    want, exp = _expect(rows, oracle_cfg, cfg)
    names = oracle_cfg.type_names
    assert [(names[f.type_id], f.start, f.end) for f in exp[0][1]] == [("CREDIT_CARD_NUMBER", 65519, 65538)]
    assert want[0][65519:65538] == FR.CARD_KA and want[0][:65519] == FILL
    data, offs = pkg("engine").pack(texts)
    n = len(texts)
    for shift in range(16):
        assert 65519 < 65536 - shift < 65538
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


@pytest.mark.parametrize("name", ["F", "FC"])
def test_corpus(name, cfgs, corpus, oracle_cfg):
    import xform_ref
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
    fell = encrypted = 0
    for i, (r, x) in enumerate(zip(rows, exp)):
        got = out[int(oo[i]):int(oo[i + 1])]
        assert got == FR.apply_transform(r[2], x[1], names, cfg), (i, r[2])
        delta = 0                                            # output position - input position
        for f in x[1]:
            fpe = FR.fpe_of(xform_ref.pick(names[f.type_id], cfg))
            piece = r[2][f.start:f.end]
            if fpe is None:
                delta += len(FR.apply_transform(piece, [xform_hash_ref._Shift(f, f.start)], names, cfg)) - len(piece)
                continue
            key = base64.b64decode(fpe["crypto_key"]["unwrapped"]["key"])
            alphabet = FR.alphabet_of(fpe)
            fell += FR.fallen_back(alphabet, piece)
            encrypted += 1
            # the reference's decrypt of the GPU's bytes restores the input
            assert FR.surrogate(key, alphabet, got[f.start + delta:f.end + delta], decrypt=True) == piece, (i, piece)
        if name == "FC":
            assert len(got) == len(r[2])
            assert FR.apply_transform(got, x[1], names, cfg, decrypt=True) == r[2]
    assert int(oo[corp.n]) == len(out)
    # no finding falls back, so the fail-closed path hides no wrong cipher (FC: the oracle's 1040 findings)
    assert fell == 0 and encrypted > 0
    if name == "FC":
        assert encrypted == sum(len(x[1]) for x in exp) == 1040


# ------------------------------------------------------------------------------------- 5 cut rows
def test_cut_row_with_findings_across_lane_cuts(cfgs, engines, oracle_cfg):
    """a small batch scans 128-byte lanes and cuts a row longer than two of them: a card number across
    byte 128, an SSN directly followed by a removed handle across byte 256"""
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
    eng = engines("F")
    res = _check_host(eng, _rows([b"short row", row, b"mail a@b.co"]), oracle_cfg, cfgs["F"][0])
    assert eng.stats()["lane_bytes"] == 128
    assert res.text(1) == row[:120] + FR.CARD_KA + row[139:248] + FR.SSN_KA + row[266:]


# --------------------------------------------------------------------------------------- 6 window
def test_window_rescan_full_and_incremental(cfgs, oracle_cfg):
    """without the flag FPE rules take the full re-scan; with incremental_transforms=True they stay incremental
    (k_win_fpe) and every window's bytes equal the full path's and the reference's"""
    from oracle import pii_oracle as O
    E, synth = pkg("engine"), pkg("synth")
    cfg = cfgs["F"][0]
    bank = synth.build_bank(400, 900, seed=41)
    corp = synth.make_corpus(40, 12, bank, seed=42)
    rows = [(int(corp.conv_slot[i]), int(corp.role[i]),
             corp.data[int(corp.offsets[i]):int(corp.offsets[i + 1])].tobytes(), int(corp.ts_us[i]))
            for i in range(corp.n)]
    # a conversation of e-mail addresses only: windows of several hundred findings
    dense = [(3000, O.ROLE_CUSTOMER, b"a@b.co " * 120, 10 + k) for k in range(6)]
    full = E.Engine(cfgs["F"][1].blob, device=0, n_conv_slots=4096)
    incr = E.Engine(cfgs["F"][1].blob, device=0, n_conv_slots=4096)
    try:
        full.window_enable(5, 32768)
        assert full.window_mode() == "full"
        incr.window_enable(5, 32768, incremental_transforms=True)
        assert incr.window_mode() == "incremental"
        store, hist, mine = O.ContextStore(), {}, {}
        names = oracle_cfg.type_names
        encrypted = 0
        for batch in (rows[:len(rows) // 2], rows[len(rows) // 2:] + dense[:2], dense[2:]):
            args = ([r[2] for r in batch], [r[0] for r in batch], [r[1] for r in batch], [r[3] for r in batch])
            res, inc = full.rescan_window(*args), incr.rescan_window(*args)
            exp = O.process_window_rows(batch, oracle_cfg, n=5, store=store, history=hist)
            assert [int(o) for o in inc.out_offsets] == [int(o) for o in res.out_offsets]
            for i, (r, (_, fs, _)) in enumerate(zip(batch, exp)):
                win = mine.setdefault(r[0], [])
                win.append(r[2])
                del win[:-5]
                assert res.text(i) == FR.apply_transform(b"\n".join(win), fs, names, cfg), (i, r)
                assert inc.text(i) == res.text(i), (i, r)
                for got in (res, inc):
                    m = got.spans["utt"] == i
                    assert [(int(s["start"]), int(s["end"]), int(s["info_type"])) for s in got.spans[m]] == [
                        (f.start, f.end, f.type_id) for f in fs]
                encrypted += sum(names[f.type_id] in FR.F_FPE for f in fs)
        assert encrypted >= 120 * (1 + 2 + 3 + 4 + 5 + 5)    # the dense conversation's windows alone
    finally:
        full.close()
        incr.close()


# -------------------------------------------------------------------------------- 7 malformed blobs
@pytest.mark.parametrize("damage, message", FD.DAMAGE, ids=FD.IDS)
def test_malformed_fpe_sections_are_rejected(damage, message, cfgs):
    E, comp = pkg("engine"), pkg("compiler")
    c = cfgs["F"][1]
    S = comp.blob_sections(c.blob)
    assert comp._sections_to_blob(S) == c.blob              # the round trip itself changes nothing
    damage(S)
    with pytest.raises(E.PiiError):
        E.Engine(comp._sections_to_blob(S), device=0, n_conv_slots=16).close()


# --------------------------------------------------------------------------------- 8 default path
def test_shipped_config_still_gives_the_type_tokens(cfgs, engines, oracle_cfg):
    rows = _rows(KNOWN_TEXTS)
    res = _check_host(engines("shipped"), rows, oracle_cfg, cfgs["shipped"][0])
    _, exp = _expect(rows, oracle_cfg, cfgs["shipped"][0])
    for i, x in enumerate(exp):
        assert res.text(i) == x[0]                          # the oracle's own "[TYPE]" redaction
    assert res.text(0) == b"card number [CREDIT_CARD_NUMBER] ok"
