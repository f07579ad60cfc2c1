"""exclusion_rule.regex / .dictionary / .exclude_by_hotword in the rule compiler: every form and matching
type compiles to var.xt_* / xt.* beside the general exclusion sections (general mode, window_ok = 0), each
field the compiler does not take raises a RuleError naming it, and every compiled rule automaton, stepped
the way the engine steps it (text_excl_sim), agrees with `re` on quotes of the synth bank and on hand-made
edge cases.  (Before text exclusion rules every config here was the RuleError "exclusion_rule.<form> is not
supported".)"""
import os
import re

import numpy as np
import pytest
import yaml

import text_excl_configs as TC
import text_excl_ref as TR
import text_excl_rows as TRW
from conftest import ROOT, pkg
from text_excl_sim import TextExclSim, XT_FULL, XT_HOTWORD, XT_INVERSE, XT_SEARCH


@pytest.fixture(scope="module")
def builtin():
    with open(os.path.join(pkg("compiler").RULES_DIR, "builtin_infotypes.yaml")) as f:
        return yaml.safe_load(f)


def _compile(cfg, builtin):
    comp = pkg("compiler")
    return comp.compile_rules(comp.Rules(cfg, builtin), text_exclusions=True)


@pytest.fixture(scope="module")
def compiled_cfgs(builtin):
    return {n: _compile(getattr(TC, n)(), builtin) for n in ("all_forms", "hand", "text_only", "context_cfg")}


def _one(rule, types=("EMAIL_ADDRESS",)):
    return TC.with_rules([TC.rule_set(list(types), rule)])


# ------------------------------------------------------------------------------------------- forms
FORMS = [("regex", TC.by_regex, r"@acme\.com", "@acme\\.com"),
         ("dictionary", TC.by_dictionary, ["acme", "Example.com"], r"(?i)\b(?:acme|Example\.com)\b")]


@pytest.mark.parametrize("form, make, arg, pat", FORMS, ids=[f[0] for f in FORMS])
@pytest.mark.parametrize("matching, kind", [(None, XT_FULL), (TC.FULL, XT_FULL), (TC.PARTIAL, XT_SEARCH),
                                            (TC.INVERSE, XT_INVERSE)])
def test_regex_and_dictionary_compile(form, make, arg, pat, matching, kind, builtin):
    c = _compile(_one(make(arg, matching)), builtin)
    S = c.sections
    assert S["xt.rule"].reshape(-1, 4).tolist() == [[kind, 0, 0, 0]]
    sim = TextExclSim(c)
    V, T = int(S["meta"][3]), int(S["meta"][2])
    t = c.rules.type_id["EMAIL_ADDRESS"]
    for v in range(V):                                               # the rule set is in every context variant
        assert [sim.rules_of(v, x) for x in range(T)] == [[0] if x == t else [] for x in range(T)]
    rx = re.compile(pat.encode())
    for q in (b"jane@acme.com", b"@acme.com", b"acme", b"ACME", b"example.com", b"xacme", b"a", b"acme example.com"):
        want = {XT_FULL: rx.fullmatch(q) is not None, XT_SEARCH: rx.search(q) is not None,
                XT_INVERSE: rx.fullmatch(q) is None}[kind]
        assert sim.rule_drops(0, b"<" + q + b">", 1, 1 + len(q)) == want, q


def test_hotword_compiles(builtin):
    c = _compile(_one(TC.by_hotword(r"(?i)test card", before=20, after=10)), builtin)
    assert c.sections["xt.rule"].reshape(-1, 4).tolist() == [[XT_HOTWORD, 20, 10, 0]]
    sim = TextExclSim(c)
    assert sim.rule_drops(0, b"my Test Card 4111", 13, 17) and not sim.rule_drops(0, b"my Test Cart 4111", 13, 17)
    assert sim.rule_drops(0, b"4111 test card", 0, 4) and not sim.rule_drops(0, b"4111 a test card", 0, 4)       # (10 bytes after)


def test_general_mode_and_full_window(compiled_cfgs):
    """a config with a text rule is general: its exclude_info_types lists are in var.xg_*, the streaming lists
    are empty and the window re-scan is FULL -- even where the lists alone would stream (the shipped handle rule)"""
    for name, c in compiled_cfgs.items():
        S = c.sections
        assert all(k in S for k in ("var.xg_off", "var.xg_ids", "det.xgidx", "var.xt_off", "var.xt_ids", "xt.rule",
                                    "xt.desc", "xt.trans", "xt.flags", "xt.cmap")), name
        assert int(S["meta"][13]) == 0, name
        assert not S["var.excl_off"].any() and (S["det.exidx"] == 0xFF).all(), name
        V, T = int(S["meta"][3]), int(S["meta"][2])
        assert S["var.xt_off"].dtype == np.uint32 and S["var.xt_off"].shape == (V * T + 1,)
        assert S["var.xt_ids"].dtype == np.uint16 and len(S["var.xt_ids"]) == int(S["var.xt_off"][-1]) > 0
        n = len(S["xt.rule"]) // 4
        assert S["xt.desc"].shape == (8 * n,) and S["xt.cmap"].shape == (256 * n,) and S["var.xt_ids"].max() < n
        assert (int(S["var.xg_off"][-1]) == 0) == (name == "text_only")
    names = compiled_cfgs["all_forms"].rules.type_names
    S = compiled_cfgs["all_forms"].sections
    e, h = names.index("EMAIL_ADDRESS"), names.index("SOCIAL_HANDLE")
    assert S["var.xg_ids"][S["var.xg_off"][h]:S["var.xg_off"][h + 1]].tolist() == [e]


def test_rules_are_shared_and_ordered(builtin):
    """one rule in two rule sets is compiled once; a type's list keeps the rule sets' order"""
    a, b = TC.by_regex("x+y"), TC.by_hotword("z", after=3)
    c = _compile(TC.with_rules([TC.rule_set(["EMAIL_ADDRESS", "PHONE_NUMBER"], a, b), TC.rule_set(["PHONE_NUMBER"], b, a)]),
                 builtin)
    sim = TextExclSim(c)
    assert len(sim.rule) == 2
    assert sim.rules_of(0, c.rules.type_id["EMAIL_ADDRESS"]) == [0, 1]
    assert sim.rules_of(0, c.rules.type_id["PHONE_NUMBER"]) == [0, 1, 1, 0]


def test_a_config_without_text_rules_has_no_sections(compiled):
    assert not any(k.startswith("xt.") or k.startswith("var.xt_") for k in compiled.sections)


def test_kinds_mirror_the_engine():
    comp = pkg("compiler")
    with open(os.path.join(ROOT, "context-based-pii_amd", "csrc", "pii_layout.h")) as f:
        src = f.read()
    m = re.search(r"enum \{ XT_SEARCH = (\d), XT_FULL = (\d), XT_INVERSE = (\d), XT_HOTWORD = (\d), XT_KINDS = (\d) \}", src)
    assert m and [int(x) for x in m.groups()] == [comp.XT_SEARCH, comp.XT_FULL, comp.XT_INVERSE, comp.XT_HOTWORD, 4]
    assert (XT_SEARCH, XT_FULL, XT_INVERSE, XT_HOTWORD) == (comp.XT_SEARCH, comp.XT_FULL, comp.XT_INVERSE, comp.XT_HOTWORD)


# ----------------------------------------------------------------------------------------- refusals
HOT = {"hotword_regex": {"pattern": "test"}, "proximity": {"window_before": 10}}
REFUSED = [
    ({"regex": {"pattern": "a", "group_indexes": [1]}}, r"exclusion_rule\.regex\.group_indexes"),
    ({"regex": {"pattern": "a*"}}, "can match the empty string"),
    ({"regex": {"pattern": r"\b"}, "matching_type": TC.PARTIAL}, "can match the empty string"),
    ({"dictionary": {"cloud_storage_path": {"path": "gs://bucket/words.txt"}}}, r"exclusion_rule\.dictionary\.cloud_storage_path"),
    ({"dictionary": {"word_list": {"words": []}}}, r"exclusion_rule\.dictionary\.word_list\.words is empty"),
    ({"dictionary": {}}, r"exclusion_rule\.dictionary\.word_list\.words is empty"),
    ({"dictionary": {"word_list": {"words": ["ok", "café"]}}}, r"exclusion_rule\.dictionary\.word_list\.words: 'café' is not ASCII"),
    ({"exclude_by_hotword": {"hotword_regex": {"pattern": "test"}}}, r"exclusion_rule\.exclude_by_hotword\.proximity has no window"),
    ({"exclude_by_hotword": {"hotword_regex": {"pattern": "test"}, "proximity": {"window_before": 0, "window_after": 0}}},
     r"exclusion_rule\.exclude_by_hotword\.proximity has no window"),
    ({"exclude_by_hotword": {"hotword_regex": {"pattern": "test", "group_indexes": [0]}, "proximity": {"window_after": 4}}},
     r"exclusion_rule\.exclude_by_hotword\.hotword_regex\.group_indexes"),
    ({"exclude_by_hotword": {"hotword_regex": {"pattern": "x?"}, "proximity": {"window_after": 4}}}, "can match the empty string"),
    ({"regex": {"pattern": "a"}, "matching_type": "MATCHING_TYPE_UNSPECIFIED"}, "unknown matching_type MATCHING_TYPE_UNSPECIFIED"),
    ({"regex": {"pattern": "a"}, "exclude_by_hotword": HOT}, "exclusion_rule with regex and exclude_by_hotword"),
    ({"exclude_info_types": {"info_types": [{"name": "PHONE_NUMBER"}]}, "matching_type": TC.INVERSE},
     "unknown matching_type MATCHING_TYPE_INVERSE_MATCH"),
    ({}, "exclusion_rule with none of"),
]


@pytest.mark.parametrize("ex, message", REFUSED, ids=[str(i) for i in range(len(REFUSED))])
def test_refused_fields_are_named(ex, message, builtin):
    with pytest.raises(pkg("compiler").RuleError, match=message):
        _compile(_one({"exclusion_rule": ex}), builtin)


@pytest.mark.parametrize("rule", [TC.by_regex("@acme"), TC.by_dictionary(["acme"]), TC.by_hotword("test", before=10)],
                         ids=["regex", "dictionary", "exclude_by_hotword"])
def test_compile_rules_takes_the_forms_only_on_request(rule, builtin, tmp_path):
    """compile_rules without text_exclusions keeps its contract (the RuleError naming the form);
    compile_default, the service's entry point, compiles the same config"""
    comp = pkg("compiler")
    form = next(iter(rule["exclusion_rule"]))
    with pytest.raises(comp.RuleError, match=r"exclusion_rule\.%s is not supported" % form):
        comp.compile_rules(comp.Rules(_one(rule), builtin))
    c = comp.compile_default(TC.write(tmp_path, "one_" + form, _one(rule)))
    assert len(c.sections["xt.rule"]) == 4 and int(c.sections["meta"][13]) == 0
    assert c.blob == _compile(_one(rule), builtin).blob


def test_external_type_is_refused(builtin):
    ext = builtin["external_types"][0]
    with pytest.raises(pkg("compiler").RuleError, match="external type %s cannot be named" % ext):
        _compile(_one(TC.by_regex("a"), types=(ext,)), builtin)


# ------------------------------------------------------------------------------------------- tables
def _py_rules(cfg):
    """the text rules of a config in the compiler's order (first appearance over the variants = over the base
    rule sets: the context merge adds none), as text_excl_ref.TextRule"""
    out, seen = [], set()
    for rs in cfg["inspect_config"]["rule_set"]:
        for rule in rs["rules"]:
            if TR.is_text_rule(rule):
                key = repr(sorted(rule["exclusion_rule"].items()))
                if key not in seen:
                    seen.add(key)
                    out.append(TR.TextRule(rule["exclusion_rule"]))
    return out


def _quotes(n_rows=600):
    """(row, s, e): every finding-shaped span of synth rows -- the oracle's findings under the shipped rules,
    with and without context -- plus digit runs and words, so each automaton sees quotes of every type"""
    from oracle import pii_oracle as O
    ocfg = O.RuleConfig.load()
    out = []
    for t in pkg("synth").build_bank(100, n_rows, seed=41).texts:
        spans = {(f.start, f.end) for et in (None, "CVV_NUMBER", "FINANCIAL_ACCOUNT_NUMBER") for f in O.find_pii(t, ocfg, et)}
        spans |= {m.span() for m in re.finditer(rb"\d[\d /.-]*\d|[A-Za-z]+(?: [A-Za-z]+)?", t[:200])}
        out += [(t, s, e) for s, e in sorted(spans)]
    return out


EDGES = [  # (row, s, e)
    (b"x", 0, 1), (b"#", 0, 1), (b"a#b", 1, 2),                                     # one-byte quotes
    (b"xORD-01234x", 1, 10), (b"ORD-01234", 0, 9), (b"xRedx", 1, 4), (b"dark red", 0, 8), (b"darkred", 0, 7),   # \b at a quote edge
    (b"a RED b", 2, 5), (b"a rEd b", 2, 5), (b"DARK red", 0, 8), (b"TEAL", 0, 4),     # case folding
    (b"sample TK11111", 7, 14), (b"ample TK11111", 6, 13), (b"TK11111", 0, 7),        # hotword window clipped at the row start
    (b"a sample TK1", 9, 12), (b"xsample TK1", 8, 11), (b"SAMPLE  TK1", 8, 11),
    (b"BG1234 void", 0, 6), (b"BG1234 voi", 0, 6), (b"BG1234void", 0, 6), (b"BG1234", 0, 6),   # ... and at the row end
    (b"BG1234 a void b", 0, 6), (b"BG1234 avoid", 0, 6), (b"BG1234voids", 0, 6),
    (b"jane@example.com", 0, 16), (b"jane@example.community", 0, 22), (b"(212) 555-0187", 0, 14), (b"01/02/1990", 0, 10),
    (b"xzbb zbb", 0, 4), (b"xzbb zbb", 5, 8), (b"# % #", 0, 1), (b"# % #", 2, 3), (b"zip z00000-1234 ok", 4, 15),
    (b"REF TST 123456", 0, 14), (b"see ORD-9912", 4, 12), (b"call 800-555-0187", 5, 17), (b"212-555-0187", 0, 12),
    (b"10.1.2.3", 0, 8), (b"110.1.2.3", 0, 9), (b"000012345678", 0, 12), (b"fax 212-555-0187", 4, 16), (b"faxes 212-555-0187", 6, 18),
    (b"12 Oak Street", 0, 13), (b"12 oaks Street", 0, 14), (b"card number 4111111111111111 thanks", 12, 28),
]


@pytest.mark.parametrize("name", ["all_forms", "hand", "context_cfg"])
def test_rule_automata_agree_with_re(name, compiled_cfgs):
    c = compiled_cfgs[name]
    sim, rules = TextExclSim(c), _py_rules(getattr(TC, name)())
    assert len(rules) == len(sim.rule)
    kinds = {("regex", TC.FULL): XT_FULL, ("regex", TC.PARTIAL): XT_SEARCH, ("regex", TC.INVERSE): XT_INVERSE,
             ("dictionary", TC.FULL): XT_FULL, ("dictionary", TC.PARTIAL): XT_SEARCH, ("dictionary", TC.INVERSE): XT_INVERSE}
    for h, r in enumerate(rules):
        assert int(sim.rule[h][0]) == (XT_HOTWORD if r.form == "exclude_by_hotword" else kinds[(r.form, r.matching)])
    cases = EDGES + [(t, 0, len(t)) for t, _ in TRW.HAND] + _quotes()
    fired = [0] * len(rules)
    for text, s, e in cases:
        for h, r in enumerate(rules):
            want = r.drops(text, s, e)
            assert sim.rule_drops(h, text, s, e) == want, (name, h, text, s, e)
            fired[h] += want
    assert all(fired) and all(f < len(cases) for f in fired), " ".join(map(str, fired))         # every rule both drops and keeps


def test_lists_follow_the_context_variants(compiled_cfgs):
    """(variant, type) lists agree with the reference's rule sets of that variant"""
    from oracle import pii_oracle as O
    for name in ("hand", "context_cfg"):
        c = compiled_cfgs[name]
        sim = TextExclSim(c)
        groups = [t for t, _, _ in c.rules.kw_groups]
        rules = _py_rules(getattr(TC, name)())
        key = lambda r: (r.form, r.matching, getattr(r, "regex", None) and r.regex.pattern,
                         getattr(r, "hot", None) and (r.hot.pattern, r.hot.window_before, r.hot.window_after))
        index = {key(r): h for h, r in enumerate(rules)}
        ref = TR.Ref(O.RuleConfig(getattr(TC, name)(), yaml.safe_load(open(os.path.join(pkg("compiler").RULES_DIR,
                                                                                        "builtin_infotypes.yaml")))))
        for v, et in enumerate([None] + groups):
            want = {}
            for types, _, by_text in ref.rule_sets(et):
                for t in types:
                    if t in c.rules.type_id:
                        want.setdefault(c.rules.type_id[t], []).extend(index[key(r)] for r in by_text)
            for t in range(sim.T):
                assert sim.rules_of(v, t) == want.get(t, []), (name, v, t)


def test_known_answers_hold_in_the_reference(tmp_path):
    """the literal rows of text_excl_rows under the reference (the GPU tests compare the engine with both)"""
    from oracle import pii_oracle as O
    ref = TR.Ref(O.RuleConfig.load(TC.write(tmp_path, "hand", TC.hand())))
    for t, want in TRW.HAND:
        assert ref.redact(t)[0] == want, t
    ref = TR.Ref(O.RuleConfig.load(TC.write(tmp_path, "ctx", TC.context_cfg())))
    for t, et, want in TRW.CONTEXT:
        assert ref.redact(t, et)[0] == want, (t, et)
