"""The incremental window re-scan under mask, keep and hash transformations (PII_WINDOW_XF) on the GPU.

An engine enabled with the flag must give, window for window, what an engine in the FULL re-scan gives and
what the references give: the oracle's findings of "\\n".join(window) (window_ext_ref where a row carries
external candidates) through xform_hash_ref.apply_transform.  Every row of every call is compared.

Configs: A, B, C (xform_configs), H, HC (xform_hash_ref), D (replace / remove only), the shipped block, and
MH = SSN masked from the end, PERSON_NAME masked, e-mail hashed, the rest "[TYPE]" -- the one block with a
masked and a hashed kind, for the tests that need both in one window.  Needs an MI355X: pytest -m gpu."""
import copy
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import window_ext_ref as WR
import xform_configs as X
import xform_hash_ref as HR
import xform_ref
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu

D = [{"info_types": [{"name": "EMAIL_ADDRESS"}],
      "primitive_transformation": {"replace_config": {"new_value": {"string_value": "<email>"}}}},
     {"info_types": [{"name": "SOCIAL_HANDLE"}], "primitive_transformation": {"redact_config": {}}},
     {"primitive_transformation": {"replace_with_info_type_config": {}}}]
SSN_MASK = {"character_mask_config": {"masking_character": "*", "number_to_mask": 4, "reverse_order": True}}
MH = [{"info_types": [{"name": "US_SOCIAL_SECURITY_NUMBER"}], "primitive_transformation": SSN_MASK},
      {"info_types": [{"name": "PERSON_NAME"}], "primitive_transformation": X.KNOWN_EXT[0][0]},
      {"info_types": [{"name": "EMAIL_ADDRESS"}], "primitive_transformation": HR.hash_prim(HR.KEY1)},
      {"primitive_transformation": {"replace_with_info_type_config": {}}}]
BLOCKS = {"A": X.A, "B": X.B, "C": X.C, "D": D, "H": HR.H, "HC": HR.HC, "MH": MH, "shipped": None}
PIECE_MAX = 1024                     # k_win_redact's LDS piece table: 2 pieces per finding + 2 per entry


@pytest.fixture(scope="module")
def cfgs(tmp_path_factory):
    """name -> (config dict, compiled rules), compiled from a JSON file as a user's config would be"""
    comp = pkg("compiler")
    d = tmp_path_factory.mktemp("winxf")
    out = {}

    def get(name):
        if name not in out:
            cfg = X.with_block(BLOCKS[name])
            out[name] = (cfg, comp.compile_default(X.write(d, name, cfg)))
        return out[name]
    return get


def _engine(blob, xf, full=False, slot_bytes=65536, n_slots=4096):
    e = pkg("engine").Engine(blob, device=0, n_conv_slots=n_slots)
    try:
        e.window_enable(5, slot_bytes, full=full, incremental_transforms=xf)
    except Exception:
        e.close()
        raise
    return e


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


class _Ref:
    """the references over a stream of calls: per call [(joined window, findings, context type)]"""

    def __init__(self, ocfg):
        from oracle import pii_oracle as O
        self.ocfg, self.state = ocfg, (O.ContextStore(), {})

    def call(self, rows, ext=None):
        ext = ext if ext is not None else [[] for _ in rows]
        return WR.process_window_rows_ext(rows, ext, self.ocfg, n=5, store=self.state[0], history=self.state[1])

    def windows(self, rows, ext=None):
        """process the call row by row, so that each row's joined window is at hand"""
        out = []
        for i, r in enumerate(rows):
            (red, fs, et), = self.call([r], None if ext is None else [ext[i]])
            out.append((b"\n".join(t for t, _ in self.state[1][r[0]]), fs, et))
        return out


def _check(res, wins, ocfg, cfg, rows):
    """one call's result against the references: bytes, offsets, spans, context group; no placeholder"""
    groups = list(ocfg.context_keywords.keys())
    want = [HR.apply_transform(j, fs, ocfg.type_names, cfg) for j, fs, _ in wins]
    for i, w in enumerate(want):
        assert res.text(i) == w, (i, rows[i], res.text(i)[:120], w[:120])
        assert HR.PLACEHOLDER not in res.text(i)
        g = int(res.ctx_info[i])
        assert (groups[g] if g >= 0 else None) == wins[i][2], (i, rows[i])
    assert [int(o) for o in res.out_offsets] == [0] + [int(x) for x in np.cumsum([len(w) for w in want])]
    assert _spans(res) == [(i, f.start, f.end, f.type_id, f.likelihood) for i, (_, fs, _) in enumerate(wins) for f in fs]


# ------------------------------------------------------------------------------------------ 1 mode
def test_mode(cfgs, oracle_cfg):
    E = pkg("engine")
    for name in ("A", "B", "C", "H", "HC"):
        eng = E.Engine(cfgs(name)[1].blob, device=0, n_conv_slots=16)
        try:
            eng.window_enable(5, 4096, incremental_transforms=True)
            assert eng.window_mode() == "incremental", name
            eng.window_enable(5, 4096, full=True, incremental_transforms=True)
            assert eng.window_mode() == "full", name
            if name in ("A", "B", "H"):
                eng.window_enable(5, 4096)
                assert eng.window_mode() == "full", name
            assert eng.lib.pii_window_enable_ex(eng.h, 5, 4096, 4) == E.PII_E_ARG
            assert eng.lib.pii_window_enable_ex(eng.h, 5, 4096, 2 | 4) == E.PII_E_ARG
        finally:
            eng.close()


@pytest.mark.parametrize("name", ["D", "shipped"])
def test_flag_changes_nothing_without_such_types(name, cfgs, oracle_cfg):
    cfg, comp = cfgs(name)
    a, b = _engine(comp.blob, False), _engine(comp.blob, True)
    try:
        assert a.window_mode() == b.window_mode() == "incremental"
        for rows, w in zip(*_corpus_calls()):
            ra, rb = _call(a, rows), _call(b, rows)
            _same(ra, rb, len(rows))
            _check(rb, w, oracle_cfg, cfg, rows)
        assert (a.histogram() == b.histogram()).all()
    finally:
        a.close()
        b.close()


def test_rules_the_incremental_path_cannot_take_stay_full(tmp_path):
    import excl_configs
    E, comp = pkg("engine"), pkg("compiler")
    block = {"info_type_transformations": {"transformations": X.A}}
    # a detector whose \s can consume the "\n" join
    nl = copy.deepcopy(X.with_block(X.A))
    nl["inspect_config"]["custom_info_types"].append(
        {"info_type": {"name": "ORDER_REFERENCE"}, "regex": {"pattern": "\\border\\s+ref\\s*:?\\s*\\d{6}\\b"},
         "likelihood": "VERY_LIKELY"})
    # general exclusion rules (PARTIAL_MATCH of custom types)
    gen = excl_configs.g1()
    gen["deidentify_config"] = block
    for name, cfg in (("newline", nl), ("general", gen)):
        eng = E.Engine(comp.compile_default(X.write(tmp_path, name, cfg)).blob, device=0, n_conv_slots=16)
        try:
            if name == "general":
                assert eng.exclusion_mode() == 1
            eng.window_enable(5, 4096, incremental_transforms=True)
            assert eng.window_mode() == "full", name
        finally:
            eng.close()


# ------------------------------------------------------------------------------ 2 literal known answers
KNOWN_A_OUT = [b"my ssn is 536-22-**** thanks", b"card number #### #### #### 1111 ok", b"card number ####-####-####-1111",
               b"reach me at <email> or ***-***-****", b"", b"A1234567", b"ip address 10.20.30.40"]


def test_known_answers_under_a(cfgs, oracle_cfg):
    from oracle import pii_oracle as O
    assert KNOWN_A_OUT == [o for _, o in X.KNOWN_A]
    cfg, comp = cfgs("A")
    eng = _engine(comp.blob, True)
    try:
        assert eng.window_mode() == "incremental"
        ref = _Ref(oracle_cfg)
        for i, (text, _) in enumerate(X.KNOWN_A):
            rows = [(7, O.ROLE_OTHER, text, 10 + i)]
            res = _call(eng, rows)
            assert res.text(0) == b"\n".join(KNOWN_A_OUT[max(0, i - 4):i + 1]), i
            _check(res, ref.windows(rows), oracle_cfg, cfg, rows)
    finally:
        eng.close()


def test_known_surrogates_under_h(cfgs, oracle_cfg):
    from oracle import pii_oracle as O
    cfg, comp = cfgs("H")
    eng = _engine(comp.blob, True)
    try:
        ref = _Ref(oracle_cfg)
        rows = [(3, O.ROLE_CUSTOMER, b"card number " + HR.CARD + b" ok", 1), (3, O.ROLE_CUSTOMER, b"thanks", 2),
                (3, O.ROLE_CUSTOMER, b"my ssn is " + HR.SSN, 3)]
        res = _call(eng, rows[:2])
        _check(res, ref.windows(rows[:2]), oracle_cfg, cfg, rows[:2])
        assert res.text(0) == b"card number " + HR.CARD_KEY1 + b" ok"
        res = _call(eng, rows[2:])
        _check(res, ref.windows(rows[2:]), oracle_cfg, cfg, rows[2:])
        assert res.text(0) == b"card number " + HR.CARD_KEY1 + b" ok\nthanks\nmy ssn is " + HR.SSN_KEY1
    finally:
        eng.close()


# ---------------------------------------------------------------- 3 differential and reference stream
DENSE_MAIL = b"a@b.co " * 120
DENSE_PHONE = b"212-555-0187 " * 100


@functools.lru_cache(maxsize=None)
def _corpus_calls():
    """test_window_rescan's corpus plus two dense conversations, in three calls; the references' windows
    (config independent: the oracle ignores deidentify_config), computed once"""
    from oracle import pii_oracle as O
    synth = pkg("synth")
    ocfg = O.RuleConfig.load()
    bank = synth.build_bank(400, 900, seed=41)
    corp = synth.make_corpus(40, 12, bank, seed=42)
    rows = [(int(corp.conv_slot[i]), int(corp.role[i]),
             corp.data[int(corp.offsets[i]):int(corp.offsets[i + 1])].tobytes(), int(corp.ts_us[i]))
            for i in range(corp.n)]
    mail = [(3000, O.ROLE_CUSTOMER, DENSE_MAIL, 10 + k) for k in range(6)]
    phone = [(3001, O.ROLE_CUSTOMER, DENSE_PHONE, 10 + k) for k in range(6)]
    half = len(rows) // 2
    calls = [rows[:half], rows[half:] + mail[:2] + phone[:2], mail[2:] + phone[2:]]
    ref = _Ref(ocfg)
    return calls, [ref.windows(c) for c in calls]


def test_the_constructed_rows_hold_what_they_are_meant_to():
    """(no GPU work) the dense windows overflow the piece table with the kinds under test, the ordinary
    tiles do not and hold such findings too: the staged and the slow path both run with SRC"""
    from oracle import pii_oracle as O
    ocfg = O.RuleConfig.load()
    names = ocfg.type_names
    calls, wins = _corpus_calls()
    last_mail, last_phone = wins[2][3], wins[2][7]
    assert calls[2][3][0] == 3000 and calls[2][7][0] == 3001
    assert [names[f.type_id] for f in last_mail[1]] == ["EMAIL_ADDRESS"] * 600
    assert [names[f.type_id] for f in last_phone[1]] == ["PHONE_NUMBER"] * 500
    # (a workgroup's windows share the table: the last call is one tile, the second call's last tile holds
    # the dense conversations' first rows)
    pieces = lambda ws: sum(2 * len(fs) + 2 * (j.count(b"\n") + 1) - 1 for j, fs, _ in ws)     # noqa: E731
    assert len(calls[2]) <= 16 and pieces(wins[2][4:]) > PIECE_MAX and pieces(wins[2][:4]) > PIECE_MAX
    assert pieces(wins[1][len(wins[1]) // 64 * 64:]) > PIECE_MAX and calls[1][-1][0] == 3001
    # the other 64-window tiles fit the table, and hold card and phone numbers (A, B, C: masked) and e-mail
    # addresses (H, HC: hashed) as well
    fit = [wins[c][t:t + 64] for c in (0, 1) for t in range(0, len(wins[c]), 64)][:-1]
    assert len(fit) == 7 and all(pieces(ws) <= PIECE_MAX for ws in fit)
    kinds = {names[f.type_id] for ws in fit for _, fs, _ in ws for f in fs}
    assert {"PHONE_NUMBER", "EMAIL_ADDRESS", "CREDIT_CARD_NUMBER"} <= kinds, kinds


@pytest.mark.parametrize("name", ["A", "B", "C", "H", "HC"])
def test_stream_equals_the_full_rescan_and_the_references(name, cfgs, oracle_cfg):
    cfg, comp = cfgs(name)
    calls, wins = _corpus_calls()
    full, inc = _engine(comp.blob, False, full=True), _engine(comp.blob, True)
    try:
        assert (full.window_mode(), inc.window_mode()) == ("full", "incremental")
        for rows, w in zip(calls, wins):
            rf, ri = _call(full, rows), _call(inc, rows)
            _same(rf, ri, len(rows))
            _check(ri, w, oracle_cfg, cfg, rows)
        assert (full.histogram() == inc.histogram()).all()
    finally:
        full.close()
        inc.close()


# ------------------------------------------------------------ 4 the three text sources, the ring wrap
# A 60-byte row enters the ring as 64 bytes of text and 16 bytes per resident candidate (several patterns
# match an SSN): window_enable(5, 512) with rows of 60 to 100 bytes cannot hold a five-row window, the calls
# end in PII_E_NOMEM (measured, also at 640).  800 bytes hold five entries of 96 to 160 bytes and never all
# nineteen, one after the other: whichever size the entries have, one of rows six to nine finds no room
# behind the newest entry and is placed at arena offset 0, and so is every fifth to eighth row after it.
SMALL_SLOT = 800


def _mh_row(k, n=60):
    """an n-byte row with an SSN (masked from the end) and an e-mail address (hashed), shifted by k"""
    head = b"w" * (k % 7) + b" "
    body = head + b"ssn 536-22-%04d mail u%d@b.co " % (1000 + k, k % 10)
    return body + b"f" * (n - len(body))


def _three_sources_stream():
    from oracle import pii_oracle as O
    C = O.ROLE_CUSTOMER
    calls = [[(5, C, _mh_row(k), 1 + k)] for k in range(4)]
    calls.append([(5, C, _mh_row(k), 1 + k) for k in range(4, 7)])
    calls += [[(5, C, _mh_row(k), 1 + k)] for k in range(7, 19)]
    return calls


def test_ring_entries_batch_predecessors_and_the_row(cfgs, oracle_cfg):
    from oracle import pii_oracle as O
    names = oracle_cfg.type_names
    assert all(60 <= len(_mh_row(k)) <= 100 for k in range(19))
    for k in range(19):
        assert [names[f.type_id] for f in O.find_pii(_mh_row(k), oracle_cfg)] == [
            "US_SOCIAL_SECURITY_NUMBER", "EMAIL_ADDRESS"], k
    cfg, comp = cfgs("MH")
    # SMALL_SLOT: the sixth entry finds no room behind the fifth and wraps to arena offset 0
    eng = _engine(comp.blob, True, slot_bytes=SMALL_SLOT, n_slots=16)
    try:
        assert eng.window_mode() == "incremental"
        ref = _Ref(oracle_cfg)
        for rows in _three_sources_stream():
            res = _call(eng, rows)
            w = ref.windows(rows)
            _check(res, w, oracle_cfg, cfg, rows)
            if len(rows) == 3:           # its last window: two ring entries, two batch predecessors, the row
                assert len(w[2][1]) == 10 and w[2][0].count(b"\n") == 4
        assert eng.window_count(5) == 5
        # what can be observed of the wrap: every call succeeded although the entries committed one after the
        # other (at least the rows' text, each rounded up to 16 bytes) are more than the slot holds, so arena
        # space was used again; an entry is contiguous, so some entry began below its predecessor
        committed = sum((len(r[2]) + 15) // 16 * 16 for rows in _three_sources_stream() for r in rows)
        assert committed > SMALL_SLOT, committed
    finally:
        eng.close()


# ------------------------------------------------------------------------ 5 tile edges and alignment
def test_windows_straddle_the_tiles(cfgs, oracle_cfg):
    """130 conversations in one call (64-window workgroups), twice, so the second call's windows hold a ring
    entry; then 40 conversations with external candidates (16-window workgroups)"""
    from oracle import pii_oracle as O
    C = O.ROLE_CUSTOMER
    P = oracle_cfg.type_id["PERSON_NAME"]
    cfg, comp = cfgs("MH")
    eng = _engine(comp.blob, True, slot_bytes=4096, n_slots=256)
    try:
        ref = _Ref(oracle_cfg)
        for k in range(2):
            rows = [(c, C, _mh_row(c + k, 60 + c % 41), 1 + k) for c in range(130)]
            _check(_call(eng, rows), ref.windows(rows), oracle_cfg, cfg, rows)
        for k in range(2):
            rows = [(c, C, b"I am Jane Doe%d, " % c + _mh_row(c + k, 60 + c % 41), 3 + k) for c in range(40)]
            ext = [[(5, 13, P, 4)] for _ in rows]
            w = ref.windows(rows, ext)
            assert all(any(f.type_id == P for f in fs) for _, fs, _ in w)
            _check(_call(eng, rows, ext), w, oracle_cfg, cfg, rows)
    finally:
        eng.close()


def test_first_byte_last_byte_and_after_the_newline(cfgs, oracle_cfg):
    """a hashed finding (and a masked one, reverse_order) at the window's first byte, at its last byte and
    directly after a "\\n", behind 1 + p bytes of padding in the earlier entry, p = 0..15: the 44 output
    bytes start at every misalignment of the 16-byte block assembly"""
    from oracle import pii_oracle as O
    C = O.ROLE_CUSTOMER
    cfg, comp = cfgs("MH")
    pii = {0: b"a@b.co", 1: b"536-22-1234"}
    calls = [[], [], []]
    for p in range(16):
        for kind, v in pii.items():
            c = 2 * p + kind
            calls[0].append((c, C, v + b" " + b"x" * p, 1))          # first byte; then p + 1 bytes of padding
            calls[1].append((c, C, v, 2))                            # after the "\n", and the window's last byte
            calls[2].append((c, C, b"y" * p + b" " + v, 3))          # last byte
    eng = _engine(comp.blob, True, slot_bytes=4096, n_slots=64)
    try:
        ref = _Ref(oracle_cfg)
        starts = set()
        for k, rows in enumerate(calls):
            w = ref.windows(rows)
            for j, fs, _ in w:
                assert fs[0].start == 0 and len(fs) == k + 1
                if k >= 1:
                    assert fs[-1].end == len(j) and j[fs[1].start - 1:fs[1].start] == b"\n"
            res = _call(eng, rows)
            _check(res, w, oracle_cfg, cfg, rows)
            for i in range(0, len(rows), 2):                        # where the hashed windows' surrogates start
                o = int(res.out_offsets[i])
                starts |= {(o + f.start + q * (HR.HASH_LEN - len(pii[0]))) % 16 for q, f in enumerate(w[i][1])}
        assert starts == set(range(16)), starts
    finally:
        eng.close()


# --------------------------------------------------------------------- 6 context change between windows
def test_a_later_agent_row_changes_what_the_window_selects(tmp_path):
    """rules whose context variants differ (rules/context_variant.json): an account number is a finding only
    while the conversation expects one, a card number's likelihood depends on the expected type"""
    from oracle import pii_oracle as O
    E, comp = pkg("engine"), pkg("compiler")
    with open(os.path.join(ROOT, "context-based-pii_amd", "rules", "context_variant.json")) as f:
        cfg = json.load(f)
    cfg["deidentify_config"] = {"info_type_transformations": {"transformations": [
        {"info_types": [{"name": "CREDIT_CARD_NUMBER"}], "primitive_transformation": X.CARD_MASK},
        {"info_types": [{"name": "FINANCIAL_ACCOUNT_NUMBER"}], "primitive_transformation": HR.hash_prim(HR.KEY1)},
        {"primitive_transformation": {"replace_with_info_type_config": {}}}]}}
    path = X.write(tmp_path, "ctxvar", cfg)
    ocfg = O.RuleConfig.load(path)
    A, C = O.ROLE_AGENT, O.ROLE_CUSTOMER
    rows = [(9, A, b"what is your account number", 1_000_000), (9, C, b"it is 987654321 ok", 2_000_000),
            (9, C, b"card 4141-1212-2323-5009", 3_000_000), (9, A, b"and your card number please", 4_000_000),
            (9, C, b"thanks", 5_000_000)]
    eng = _engine(comp.compile_default(path).blob, True, n_slots=16)
    try:
        assert eng.window_mode() == "incremental"
        ref = _Ref(ocfg)
        seen = []
        for r in rows:
            w = ref.windows([r])
            _check(_call(eng, [r]), w, ocfg, cfg, [r])
            seen.append((w[0][2], [(ocfg.type_names[f.type_id], f.likelihood) for f in w[0][1]]))
        assert seen[2] == ("FINANCIAL_ACCOUNT_NUMBER", [("FINANCIAL_ACCOUNT_NUMBER", 5), ("CREDIT_CARD_NUMBER", 4)])
        assert seen[3] == ("CREDIT_CARD_NUMBER", [("CREDIT_CARD_NUMBER", 5)])
        assert seen[4] == seen[3]
    finally:
        eng.close()


# -------------------------------------------------------------------------------- 7 external candidates
@pytest.mark.parametrize("which", ["mask_utf8", "mask_reverse", "hash"] + ["long_" + k for k in sorted(X.LONG_MASKS)])
def test_external_candidates(which, cfgs, oracle_cfg, tmp_path):
    """long_*: the rows of test_gpu_transform's test_masked_candidate_of_several_windows_at_every_alignment, a
    68-byte candidate (the entry point does not limit its length) at 16 alignments under X.LONG_MASKS, one row
    per call; each window is also what the batch path gives for the joined window with the same candidates"""
    from oracle import pii_oracle as O
    E, comp = pkg("engine"), pkg("compiler")
    long = which.startswith("long_")
    C = O.ROLE_CUSTOMER
    P = oracle_cfg.type_id["PERSON_NAME"]
    if long:
        prim = X.LONG_MASKS[which[5:]]
        texts, at = X.long_rows()
        rows = [(4, C, t, 1 + k) for k, t in enumerate(texts)]
        ext = [[(s, e, P, 4)] for s, e in at]
        masked = xform_ref.mask(X.LONG_NAME, prim["character_mask_config"])
        want = [t[:s] + masked + t[e:] for t, (s, e) in zip(texts, at)]
    else:
        prim = {"mask_utf8": X.KNOWN_EXT[0][0], "mask_reverse": X.KNOWN_EXT[1][0],
                "hash": HR.hash_prim(HR.KEY1)}[which]
        first = {"mask_utf8": X.KNOWN_EXT[0][1], "mask_reverse": X.KNOWN_EXT[1][1],
                 "hash": b"I am " + HR.JOSE_KEY1 + b" ok"}[which]
        rows = [(4, C, X.EXT_TEXT, 1)] + [(4, C, b"row %d 212-555-0187" % k, 2 + k) for k in range(5)]
        ext = [[(X.EXT_SPAN[0], X.EXT_SPAN[1], P, 4)]] + [[] for _ in range(5)]
    cfg = X.with_block([{"info_types": [{"name": "PERSON_NAME"}], "primitive_transformation": prim},
                        {"primitive_transformation": {"replace_with_info_type_config": {}}}])
    blob = comp.compile_default(X.write(tmp_path, "ext_" + which, cfg)).blob
    full, inc = _engine(blob, False, full=True, n_slots=16), _engine(blob, True, n_slots=16)
    batch = E.Engine(blob, device=0, n_conv_slots=16) if long else None
    try:
        assert (full.window_mode(), inc.window_mode()) == ("full", "incremental")
        ref = _Ref(oracle_cfg)
        for k, (r, x) in enumerate(zip(rows, ext)):
            w = ref.windows([r], [x])
            rf, ri = _call(full, [r], [x]), _call(inc, [r], [x])
            _same(rf, ri, 1)
            _check(ri, w, oracle_cfg, cfg, [r])
            if not long:
                assert ri.text(0).startswith(first) == (k < 5), k        # five consecutive windows hold the row
                continue
            assert ri.text(0) == b"\n".join(want[max(k - 4, 0):k + 1]), k
            joined, fs, _ = w[0]
            assert [f.type_id for f in fs] == [P] * min(k + 1, 5)
            rb = batch.scan_redact([joined], [4], [C], [r[3]],
                                   ext=[[(f.start, f.end, f.type_id, f.likelihood) for f in fs]])
            assert rb.text(0) == ri.text(0) and _spans(rb) == _spans(ri), k
    finally:
        full.close()
        inc.close()
        if batch:
            batch.close()


# -------------------------------------------------------------------------- 8 nothing committed on failure
def test_capacity_and_ring_errors_commit_nothing(cfgs, oracle_cfg):
    from oracle import pii_oracle as O
    E = pkg("engine")
    cfg, comp = cfgs("MH")
    A, C = O.ROLE_AGENT, O.ROLE_CUSTOMER
    eng = _engine(comp.blob, True, slot_bytes=SMALL_SLOT, n_slots=16)
    try:
        ref = _Ref(oracle_cfg)
        rows = [(2, C, _mh_row(1), 1), (2, C, _mh_row(2), 2)]
        _check(_call(eng, rows), ref.windows(rows), oracle_cfg, cfg, rows)
        rows = [(2, A, b"What is your email address?", 3), (2, C, _mh_row(3), 4)]
        w = ref.windows(rows)
        want = [HR.apply_transform(j, fs, oracle_cfg.type_names, cfg) for j, fs, _ in w]
        need, nsp = sum(len(x) for x in want), sum(len(fs) for _, fs, _ in w)
        data, offs = E.pack([r[2] for r in rows])
        n = len(rows)
        sl, rl = np.full(n, 2, np.uint32), np.array([r[1] for r in rows], np.uint8)
        ts = np.array([r[3] for r in rows], np.int64)
        before = (eng.window_count(2), eng.context_get(2))
        assert before[0] == 2 and before[1][0] == -1

        def call(out_cap):
            out, oo = np.full(need + 64, 0xEE, np.uint8), np.zeros(n + 1, np.uint64)
            spans, ns, ctx = np.zeros(64, E.SPAN_DTYPE), ctypes.c_uint32(0), np.zeros(n, np.int16)
            p = lambda a: a.ctypes.data_as(ctypes.c_void_p)          # noqa: E731
            rc = eng.lib.pii_rescan_window(eng.h, p(data), p(offs), n, p(sl), p(rl), p(ts), p(out), out_cap, p(oo),
                                           p(spans), 64, ctypes.byref(ns), p(ctx))
            return rc, out, oo, ns.value

        rc, out, oo, ns = call(need - 1)
        assert rc == E.PII_E_CAPACITY and (int(oo[n]), ns) == (need, nsp)
        assert (eng.window_count(2), eng.context_get(2)) == before
        rc, out, oo, ns = call(need)
        assert rc == E.PII_OK and (int(oo[n]), ns) == (need, nsp)
        assert out[:need].tobytes() == b"".join(want) and (out[need:] == 0xEE).all()
        assert eng.window_count(2) == 4 and eng.group_types[eng.context_get(2)[0]] == "EMAIL_ADDRESS"
        # a row the slot cannot hold: the ring error, nothing committed
        before = (eng.window_count(2), eng.context_get(2))
        with pytest.raises(E.PiiError) as ei:
            _call(eng, [(2, C, _mh_row(4, 900), 5)])
        assert ei.value.code == E.PII_E_NOMEM
        assert (eng.window_count(2), eng.context_get(2)) == before
        rows = [(2, C, _mh_row(5), 6)]
        _check(_call(eng, rows), ref.windows(rows), oracle_cfg, cfg, rows)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------ 9 device entry point
def test_device_entry_point(cfgs, oracle_cfg):
    """test 4's stream through pii_rescan_window_device_ex with the declared base and size"""
    import torch
    E = pkg("engine")
    cfg, comp = cfgs("MH")
    dev = torch.device("cuda", 0)
    eng = _engine(comp.blob, True, slot_bytes=SMALL_SLOT, n_slots=16)
    try:
        ref = _Ref(oracle_cfg)
        for rows in _three_sources_stream():
            w = ref.windows(rows)
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
            host = d_out.cpu().numpy()
            assert (host[ob:] == 0xEE).all()

            class _R:
                out_offsets = d_oo.cpu().numpy().view(np.uint64)
                out = host[:ob]
                spans = d_sp.cpu().numpy()[:ns * 16].view(E.SPAN_DTYPE)
                ctx_info = d_ctx.cpu().numpy()

                def text(self, i):
                    return self.out[int(self.out_offsets[i]):int(self.out_offsets[i + 1])].tobytes()
            _check(_R(), w, oracle_cfg, cfg, rows)
    finally:
        eng.close()
