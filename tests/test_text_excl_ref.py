"""tests/text_excl_ref.py (the reference of the text exclusion tests) pinned to the oracle: on configs without
a regex / dictionary / exclude_by_hotword exclusion rule its findings equal oracle.find_pii's exactly, over
synth rows, the general exclusion templates and every context group."""
import os
import random

import pytest

import excl_configs as XC
import excl_rows as XR
import text_excl_ref as TR
from conftest import pkg


def _configs(tmp_dir):
    comp = pkg("compiler")
    return {"shipped": os.path.join(comp.RULES_DIR, "dlp_config.json"),
            "context_variant": os.path.join(comp.RULES_DIR, "context_variant.json"),
            "G1": XC.write(tmp_dir, "G1", XC.g1())}


@pytest.fixture(scope="module")
def texts():
    bank = pkg("synth").build_bank(150, 350, seed=23).texts
    return bank + XR.template_texts(random.Random(23), 200) + [t for t, _, _ in XC.KNOWN_G1]


@pytest.mark.parametrize("name", ["shipped", "context_variant", "G1"])
def test_reference_equals_the_oracle(name, texts, tmp_path):
    from oracle import pii_oracle as O
    path = _configs(tmp_path)[name]
    ocfg = O.RuleConfig.load(path)
    ref = TR.Ref(ocfg)
    groups = [t for t, _, _ in pkg("compiler").Rules.load(path).kw_groups]
    n = 0
    for et in [None] + groups:
        for t in texts:
            want = O.find_pii(t, ocfg, et)
            assert ref.find_pii(t, et) == want, (name, et, t)
            assert not ref.fired
            n += len(want)
    assert n > 1000                                  # (not vacuous)


def test_wrappers_equal_the_oracle(texts, tmp_path):
    from oracle import pii_oracle as O
    ocfg = O.RuleConfig.load(_configs(tmp_path)["G1"])
    ref = TR.Ref(ocfg)
    r = random.Random(5)
    rows = [(i // 8, r.choice([O.ROLE_AGENT, O.ROLE_CUSTOMER, O.ROLE_OTHER]), t, 1000 * i) for i, t in enumerate(texts[:400])]
    assert ref.process_rows(rows) == O.process_rows(rows, ocfg)
    assert ref.process_window_rows(rows, n=5) == O.process_window_rows(rows, ocfg, n=5)
