"""exclusion_rule.regex / .dictionary / .exclude_by_hotword on the GPU (k_excl_text) through the C ABI, against
the reference tests/text_excl_ref.py (the oracle with these forms; pinned to the oracle by test_text_excl_ref):
spans, redacted bytes, out_offsets and per-row context, bit-exact.  Configs: text_excl_configs; rows and
known answers: text_excl_rows.  Every config here was a RuleError of the rule compiler before these rules
("exclusion_rule.<form> is not supported").  Needs an MI355X: pytest -m gpu."""
import numpy as np
import pytest

import text_excl_configs as TC
import text_excl_ref as TR
import text_excl_rows as TRW
import xform_ref
from conftest import pkg

pytestmark = pytest.mark.gpu

CONFIGS = ("hand", "all_forms", "all_forms_masked", "text_only", "context_cfg")


@pytest.fixture(scope="module")
def cfgs(tmp_path_factory):
    """name -> (config dict, compiled rules, the reference over it)"""
    from oracle import pii_oracle as O
    comp = pkg("compiler")
    d = tmp_path_factory.mktemp("text_excl")
    out = {}
    for name in CONFIGS:
        cfg = getattr(TC, name)()
        path = TC.write(d, name, cfg)
        out[name] = (cfg, comp.compile_default(path), TR.Ref(O.RuleConfig.load(path)))
    return out


@pytest.fixture(scope="module")
def engines(cfgs):
    E = pkg("engine")
    made = {}

    def get(name):
        if name not in made:
            made[name] = E.Engine(cfgs[name][1].blob, device=0, n_conv_slots=1 << 12)
            assert made[name].exclusion_mode() == 1
        return made[name]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def random_case(cfgs, tmp_path_factory):
    """4000 synth rows under no context and under every context group, the reference's result per row
    (computed once, shared and left unchanged) and the forms whose rules dropped a candidate in it"""
    cfg, c, ref = cfgs["all_forms"]
    groups = [t for t, _, _ in c.rules.kw_groups]
    rows, contexts = TRW.random_rows(groups)
    store = TRW.oracle_store(contexts, groups)
    exp, fired = [], []
    for row in rows:
        exp.append(ref.process_rows([row], store)[0])
        fired.append(ref.fired)
    return rows, contexts, groups, tuple(exp), tuple(fired)


def _spans(res):
    return [(int(s["utt"]), int(s["start"]), int(s["end"]), int(s["info_type"]), int(s["likelihood"])) for s in res.spans]


def _check(eng, rows, exp, want, groups=None):
    """one host call: every row's bytes, the offsets, the spans, the per-row context and the histogram, bit-exact"""
    eng.histogram_reset()
    res = eng.scan_redact([r[2] for r in rows], [r[0] for r in rows], [r[1] for r in rows], [r[3] for r in rows])
    if res.out.tobytes() != b"".join(want):
        for i, w in enumerate(want):
            assert res.text(i) == w, (i, rows[i][2][:160], res.text(i)[:160], w[:160])
    assert (res.out_offsets.astype(np.int64) == np.concatenate([[0], np.cumsum([len(w) for w in want])])).all()
    assert _spans(res) == [(i, f.start, f.end, f.type_id, f.likelihood) for i, x in enumerate(exp) for f in x[1]]
    groups = eng.group_types if groups is None else groups
    assert [int(x) for x in res.ctx_info] == [groups.index(x[2]) if x[2] else -1 for x in exp]
    hist = eng.histogram()
    assert (hist == np.bincount(res.spans["info_type"].astype(np.int64), minlength=len(hist))[:len(hist)]).all()
    return res


def _other(texts):
    from oracle import pii_oracle as O
    return [(0, O.ROLE_OTHER, t, 0) for t in texts]


# ------------------------------------------------------------------------------- 1 hand-written rows
def test_hand_written_rows(cfgs, engines):
    """one row per (form x matching type); a dropped candidate that still excludes another; a dropped long
    candidate that frees a shorter one; a dropped match with its pattern's next start inside it"""
    _, _, ref = cfgs["hand"]
    eng = engines("hand")
    rows = _other([t for t, _ in TRW.HAND])
    exp = ref.process_rows(rows)
    res = _check(eng, rows, exp, [x[0] for x in exp])
    for i, (t, want) in enumerate(TRW.HAND):
        assert res.text(i) == want, t
    assert eng.exclusion_occurrences() > 0            # (ZIP9, and the shipped e-mail rule's excluders)


def test_rule_sets_under_a_context_group(cfgs, engines):
    """a rule whose type -- and so whose rule set -- exists only under its context group, and rules that hold
    in every variant, on the rule set whose variants differ"""
    from oracle import pii_oracle as O
    _, c, ref = cfgs["context_cfg"]
    eng = engines("context_cfg")
    groups = eng.group_types
    assert groups == [t for t, _, _ in c.rules.kw_groups]
    rows, contexts = [], {}
    for i, (t, et, _) in enumerate(TRW.CONTEXT):
        slot = 1 + i
        if et:
            contexts[slot] = groups.index(et)
            eng.context_set(slot, contexts[slot], 0)
        rows.append((slot, O.ROLE_CUSTOMER, t, 1000))
    exp = ref.process_rows(rows, TRW.oracle_store(contexts, groups))
    assert [x[2] for x in exp] == [et for _, et, _ in TRW.CONTEXT]
    res = _check(eng, rows, exp, [x[0] for x in exp])
    for i, (t, et, want) in enumerate(TRW.CONTEXT):
        assert res.text(i) == want, (t, et)


# ------------------------------------------------------------------------------------- 2 random rows
def test_random_rows_every_context_group(cfgs, engines, random_case, tmp_path):
    rows, contexts, groups, exp, fired = random_case
    assert len(rows) == 4000 * (1 + len(groups))
    n = TRW.decided(rows, exp, fired, cfgs["all_forms"][0], tmp_path)
    print(len(rows), "rows; rows the rules decide, in all and by the form removed:", n)
    assert n["all"] >= 200, n
    for form in TR.FORMS + ("exclude_info_types",):
        assert n[form] >= 20, n
    eng = engines("all_forms")
    assert eng.group_types == groups
    for slot, g in contexts.items():
        eng.context_set(slot, g, 0)
    _check(eng, rows, exp, [x[0] for x in exp])
    assert eng.exclusion_occurrences() > 0


# --------------------------------------------------------------------------------------- 3 cut rows
def test_cut_row(cfgs, engines):
    """one row of three 1 KiB lanes: an ORDER_ID the FULL_MATCH rule drops straddles the first boundary, a
    TICKET whose exclusion hotword lies in the lane before it starts at the second; the batch is padded past
    64 MiB so that the lanes are 1 KiB.  The same row alone is cut into 128-byte lanes."""
    _, _, ref = cfgs["hand"]
    eng = engines("hand")
    row, (p_order, p_ticket) = TRW.cut_row()
    assert p_order < 1024 < p_order + 9 and p_ticket == 2048 and 2048 < len(row) <= 3072
    red, fs = ref.redact(row)
    names = ref.cfg.type_names
    got = [(f.start, names[f.type_id]) for f in fs]
    assert (p_order, "ORDER_ID") not in got and (p_ticket, "TICKET") not in got          # both dropped ...
    assert [n for _, n in got] == ["ORDER_ID", "TICKET"]                                 # ... their twins at the end kept
    filler = (TRW.FILL * 11)[:1024].encode()
    assert ref.redact(filler) == (filler, [])
    n_fill = (64 << 20) // len(filler) + 1
    rows = _other([row] + [filler] * n_fill)
    exp = [(red, fs, None, None)] + [(filler, [], None, None)] * n_fill
    _check(eng, rows, exp, [x[0] for x in exp])
    st = eng.stats(gate=True)
    assert st["lane_bytes"] == 1024 and st["cut_rows"] == 1, st
    _check(eng, rows[:1], exp[:1], [red])
    st = eng.stats(gate=True)
    assert st["lane_bytes"] == 128 and st["cut_rows"] == 1, st


# ----------------------------------------------------------------------------------- 4 window re-scan
def test_window_rescan_is_full_and_exact(cfgs):
    E = pkg("engine")
    _, c, ref = cfgs["hand"]
    rows = TRW.window_convs()
    eng = E.Engine(c.blob, device=0, n_conv_slots=64)
    try:
        eng.window_enable(5, 8192)
        assert eng.window_mode() == "full" and eng.exclusion_mode() == 1
        res = eng.rescan_window([t for _, _, t, _ in rows], [s for s, _, _, _ in rows], [x for _, x, _, _ in rows],
                                [s for _, _, _, s in rows])
        exp = ref.process_window_rows(rows, n=5)
        # the hotword before the "\n" drops the ticket after it; the hotword after the "\n" drops the badge before it
        assert exp[1][0] == b"this is a sample\nTK12345 is mine" and exp[2][0].endswith(b"\nand [TICKET] too")
        # ... while "void" ends the window; one row later it no longer does
        assert exp[4][0].endswith(b"\nBG1234\nvoid") and exp[5][0].endswith(b"\n[BADGE]\nvoid\n[BADGE]")
        by_row = {}
        for s in res.spans:
            by_row.setdefault(int(s["utt"]), []).append((int(s["start"]), int(s["end"]), int(s["info_type"]),
                                                         int(s["likelihood"])))
        for i, (red, fs, _) in enumerate(exp):
            assert res.text(i) == red, (i, rows[i], res.text(i), red)
            assert by_row.get(i, []) == [(f.start, f.end, f.type_id, f.likelihood) for f in fs], (i, rows[i])
        assert (res.out_offsets.astype(np.int64) == np.concatenate([[0], np.cumsum([len(x[0]) for x in exp])])).all()
        assert [int(x) for x in res.ctx_info] == [-1] * len(rows)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------ 5 combined cases
def test_with_a_character_mask(cfgs, engines, random_case):
    """the all-forms rules with a character_mask_config on the card numbers: the findings are the same, the
    kept card numbers come out masked, the dropped ones as they went in"""
    rows, contexts, groups, exp, _ = random_case
    cfg, _, ref = cfgs["all_forms_masked"]
    eng = engines("all_forms_masked")
    for slot, g in contexts.items():
        eng.context_set(slot, g, 0)
    names = ref.cfg.type_names
    want = [xform_ref.apply_transform(r[2], x[1], names, cfg) if x[1] else r[2] for r, x in zip(rows, exp)]
    card = names.index("CREDIT_CARD_NUMBER")
    assert sum(1 for x in exp for f in x[1] if f.type_id == card) >= 100
    assert sum(1 for w, x in zip(want, exp) if w != x[0]) >= 100                         # (masked, not "[CREDIT_CARD_NUMBER]")
    _check(eng, rows, exp, want)


def test_without_exclude_info_types_no_occurrence_phases(cfgs, engines, random_case):
    """no exclude_info_types rule in the config: the occurrence phases are not launched (their total is 0)"""
    rows, contexts, groups, _, _ = random_case
    _, c, ref = cfgs["text_only"]
    assert int(c.sections["var.xg_off"][-1]) == 0
    eng = engines("text_only")
    rows = rows[:4000] + rows[-4000:]                    # no context, and the last context group
    g = len(groups) - 1
    eng.context_set(1 + g, g, 0)
    exp = ref.process_rows(rows, TRW.oracle_store({1 + g: g}, groups))
    assert sum(1 for r, x in zip(rows, exp) if x[0] != r[2]) >= 500
    _check(eng, rows, exp, [x[0] for x in exp])
    assert eng.exclusion_occurrences() == 0
