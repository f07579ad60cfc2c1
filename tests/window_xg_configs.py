"""Configs and rows of the PII_WINDOW_XG tests (general and text exclusion rules on the incremental window
re-scan), beside excl_configs and text_excl_configs."""
import copy
import random

import excl_configs as XC
import excl_rows as XR
from conftest import pkg


def hotword_excluder() -> dict:
    """G1 with TAIL_REF at UNLIKELY and one hotword rule set on it: the excluder of PHONE_NUMBER reaches
    min_likelihood only with "ref" in the 20 bytes before it -- in a window, possibly in the previous utterance"""
    cfg = copy.deepcopy(XC.g1())
    insp = cfg["inspect_config"]
    for c in insp["custom_info_types"]:
        if c["info_type"]["name"] == "TAIL_REF":
            c["likelihood"] = "UNLIKELY"
    insp["rule_set"].append({"info_types": [{"name": "TAIL_REF"}], "rules": [{"hotword_rule": {
        "hotword_regex": {"pattern": "(?i)ref"}, "proximity": {"window_before": 20},
        "likelihood_adjustment": {"fixed_likelihood": "VERY_LIKELY"}}}]})
    return cfg


def newline_detector() -> dict:
    """G1 plus one custom detector that consumes '\\n': its windows re-scan in FULL with or without the flag"""
    return XC.with_custom(XC.G1_RULES, custom=XC.CUSTOM + [("A_B", r"a\sb")])


def hx_rows():
    """the hotword-excluder conversations: (conv, role, text, ts), all CUSTOMER"""
    from oracle import pii_oracle as O
    C = O.ROLE_CUSTOMER
    return [(0, C, b"see ref", 1), (0, C, b"4321 #212-555-0187 ok", 2), (0, C, b"x", 3),
            (1, C, b"hello", 1), (1, C, b"4321 #212-555-0187 ok", 2)]


# row index -> (redacted window, (start, end) of its one finding, likelihood) at n = 5, from the oracle (literal)
HX_WINDOWS = {
    1: (b"see ref\n[TAIL_REF]-555-0187 ok", (8, 17), 5),
    2: (b"see ref\n[TAIL_REF]-555-0187 ok\nx", (8, 17), 5),
    4: (b"hello\n4321 #[PHONE_NUMBER] ok", (12, 24), 4),
}


def g_rows():
    """the 200 conversations x 8 rows of test_gpu_exclusion.py::test_window_rescan_is_full_and_exact"""
    from oracle import pii_oracle as O
    r = random.Random(13)
    bank = pkg("synth").build_bank(50, 300, seed=13).texts
    C = O.ROLE_CUSTOMER
    rows = []
    for conv in range(200):
        for k in range(8):
            x = r.random()
            if conv == 0:
                t = [b"hello", b"jane@acme.com", b"ok", b"536-22-1234 #212-555-0187", b"bye", b"@acme.com",
                     b"bob@acme.org", b"4111 1111 1111 1111"][k]
            elif x < 0.6:
                t = XR.template_texts(r, 1)[0]
            else:
                t = r.choice(bank)
            rows.append((conv, C, t, 1 + k))
    return rows


def load(tmp_dir, name, cfg):
    """(config dict, compiled rules, the oracle's view) of a config written as a user's file"""
    from oracle import pii_oracle as O
    path = XC.write(tmp_dir, name, cfg)
    return cfg, pkg("compiler").compile_default(path), O.RuleConfig.load(path)
