"""CPU check of the decomposition behind PII_WINDOW_XG (window_xg_sim.WindowXgSim): per window, per entry,
likelihood -> candidate -> text_drop / type_drop over the entry's resident candidates -> best per start ->
overlap, against the references on the joined window: the oracle for G1, G2 and the hotword-excluder config,
text_excl_ref.Ref for the text rules.  No GPU here."""
import random

import pytest

import excl_configs as XC
import excl_rows as XR
import text_excl_configs as TC
import text_excl_ref as TR
import text_excl_rows as TRW
import window_xg_configs as WC
from window_xg_sim import WindowXgSim


@pytest.fixture(scope="module")
def loaded(tmp_path_factory):
    d = tmp_path_factory.mktemp("winxg_sim")
    made = {}

    def get(name, make):
        if name not in made:
            _, comp, ocfg = WC.load(d, name, make())
            made[name] = (WindowXgSim(comp), ocfg)
        return made[name]
    return get


def _compare(sim, ocfg, rows, exp, n):
    """exp: the reference's [(redacted window, findings, context type)] per row"""
    groups = list(ocfg.context_keywords.keys())
    got = sim.process_window_rows(rows, [x[2] for x in exp], groups, n=n)
    for i, ((W, kept), (red, fs, _)) in enumerate(zip(got, exp)):
        assert kept == [(f.start, f.end, f.type_id, f.likelihood) for f in fs], (i, rows[i], W)
        assert sim.sim.redact(W, kept) == red, (i, rows[i])


def _hand_rows(r, templates, n_conv=6):
    """conversations of 6 rows from the given templates between filler rows"""
    from oracle import pii_oracle as O
    rows = []
    for conv in range(n_conv):
        for k in range(6):
            t = templates[(conv + k) % len(templates)](r) if k % 2 else r.choice(["ok", "hello there", ""])
            rows.append((conv, O.ROLE_CUSTOMER, t.encode(), 1 + k))
    return rows


@pytest.mark.parametrize("name", ["G1", "G2"])
def test_general_rules_against_the_oracle(name, loaded):
    from oracle import pii_oracle as O
    sim, ocfg = loaded(name, XC.CONFIGS[name])
    rows = WC.g_rows()[:8 * 12]                       # conversation 0's hand rows and eleven random ones
    rows += [(1000 + c, role, t, ts) for c, role, t, ts in _hand_rows(random.Random(5), [XR.t_domain_alone, XR.t_test_card,
                                                                                        XR.t_tail_left, XR.t_pair3_hit])]
    exp = O.process_window_rows(rows, ocfg, n=5)
    if name == "G1":
        assert exp[1][0] == b"hello\njane[OUR_DOMAIN]"
        assert exp[3][0].endswith(b"\n[US_SOCIAL_SECURITY_NUMBER] #212-555-0187")
    _compare(sim, ocfg, rows, exp, 5)


def test_rules_matter_in_those_rows(loaded, tmp_path):
    """the comparison above hides no dead rule path: on the reference alone, the windows differ from the ones
    of the config without its rule sets"""
    from oracle import pii_oracle as O
    rows = WC.g_rows()[:8 * 12]
    _, _, plain = WC.load(tmp_path, "plain", XC.g1_no_rules())
    base = O.process_window_rows(rows, plain, n=5)
    for name, least in (("G1", 40), ("G2", 1)):
        _, ocfg = loaded(name, XC.CONFIGS[name])
        exp = O.process_window_rows(rows, ocfg, n=5)
        differ = sum(1 for a, b in zip(exp, base) if a[0] != b[0])
        print(name, "windows that differ from the rule-less config's:", differ, "of", len(rows))
        assert differ >= least, (name, differ)


@pytest.mark.parametrize("n", [5, 2])
def test_hotword_excluder_across_the_join(n, loaded):
    """the excluder reaches min_likelihood only through a hotword in the PREVIOUS utterance: it excludes in the
    windows that hold that utterance and in no other, so the decision cannot be taken once at arrival"""
    from oracle import pii_oracle as O
    sim, ocfg = loaded("hx", WC.hotword_excluder)
    rows = WC.hx_rows()
    exp = O.process_window_rows(rows, ocfg, n=n)
    if n == 5:
        for i, (red, span, lik) in WC.HX_WINDOWS.items():
            assert exp[i][0] == red
            assert [(f.start, f.end, f.likelihood) for f in exp[i][1]] == [(span[0], span[1], lik)]
    else:
        # the hotword row has left row 2's window: the phone number is back (the oracle's word)
        assert exp[1][0] == WC.HX_WINDOWS[1][0]
        assert exp[2][0] == O.redact(b"4321 #212-555-0187 ok\nx", ocfg, None)[0]
        assert b"[PHONE_NUMBER]" in exp[2][0] and b"[TAIL_REF]" not in exp[2][0]
    _compare(sim, ocfg, rows, exp, n)
    # the same window through O.redact
    W, kept = sim.window_select(sim.residents([b"see ref", b"4321 #212-555-0187 ok"], 5), 0)
    red, fs = O.redact(W, ocfg, None)
    assert sim.sim.redact(W, kept) == red == WC.HX_WINDOWS[1][0]


def test_text_rules_against_their_reference(loaded):
    from oracle import pii_oracle as O
    sim, ocfg = loaded("hand", TC.hand)
    assert sim.has_xt
    rows = TRW.window_convs()
    ref = TR.Ref(ocfg)
    exp = ref.process_window_rows(rows, n=5)
    # the rows are there for the hotword windows that cross a join: both directions decide something
    assert exp[1][0] == b"this is a sample\nTK12345 is mine"            # TICKET dropped by the previous row's "sample"
    assert exp[4][0].endswith(b"BG1234\nvoid")                           # BADGE dropped by the next row's "void"
    _compare(sim, ocfg, rows, exp, 5)
    # single rows with known answers, each as a window of its own and behind a filler row
    C = O.ROLE_CUSTOMER
    rows = [(i, C, t, 1) for i, (t, _) in enumerate(TRW.HAND)]
    exp = ref.process_window_rows(rows, n=5)
    assert [x[0] for x in exp] == [w for _, w in TRW.HAND]
    _compare(sim, ocfg, rows, exp, 5)
