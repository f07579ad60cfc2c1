"""The compiler's window_xg_ok marker (meta[15]): 1 only for a rule set that lost window_ok (meta[13]) solely
to its general / text exclusion rules -- no detector consumes '\\n' or tests a text edge.  No GPU here."""
import os

import pytest

import excl_configs as XC
import text_excl_configs as TC
import window_xg_configs as WC
from conftest import pkg


def _meta(tmp_path, name, cfg):
    comp = pkg("compiler")
    return comp.compile_default(XC.write(tmp_path, name, cfg)).sections


@pytest.mark.parametrize("name, make", [("G1", XC.g1), ("G2", XC.g2), ("G3", XC.g3), ("hand", TC.hand),
                                        ("hotword_excluder", WC.hotword_excluder)])
def test_marker_set_for_general_rule_sets(name, make, tmp_path):
    S = _meta(tmp_path, name, make())
    assert "var.xg_off" in S and "var.xg_ids" in S and "det.xgidx" in S
    assert len(S["meta"]) == 16 and int(S["meta"][13]) == 0 and int(S["meta"][15]) == 1


def test_marker_clear_with_a_newline_consuming_detector(tmp_path):
    S = _meta(tmp_path, "nl", WC.newline_detector())
    assert "var.xg_off" in S
    assert int(S["meta"][13]) == 0 and int(S["meta"][15]) == 0


def test_marker_clear_for_rule_sets_that_are_not_general(compiled, tmp_path):
    comp = pkg("compiler")
    assert int(compiled.sections["meta"][13]) == 1 and int(compiled.sections["meta"][15]) == 0
    c = comp.compile_default(os.path.join(comp.RULES_DIR, "context_variant.json"))
    assert int(c.sections["meta"][13]) == 1 and int(c.sections["meta"][15]) == 0
    # a '\n'-consuming detector without general rules: FULL, and no marker
    S = _meta(tmp_path, "nl_plain", XC.with_custom([], custom=[("A_B", r"a\sb")]))
    assert "var.xg_off" not in S and int(S["meta"][13]) == 0 and int(S["meta"][15]) == 0
