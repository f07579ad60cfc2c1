"""The host rule preparation (csrc/pii_rules_host.h) over blobs with text exclusion sections (var.xt_* /
xt.*), on its own: the stand-alone program of test_rules_host (tests/rules_host_main.cpp, built with the
host compiler under the address and undefined-behaviour sanitizers) accepts the blobs of text_excl_configs
and rejects, each defect with its own message, blobs whose sections are damaged one at a time."""
import os

import numpy as np
import pytest
import yaml

import text_excl_configs as TC
import rules_host_runner
from conftest import pkg

SECTIONS = ("var.xt_off", "var.xt_ids", "xt.rule", "xt.desc", "xt.trans", "xt.flags", "xt.cmap")
GOOD = ("all_forms", "hand", "text_only", "context_cfg")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    return rules_host_runner.runner(tmp_path_factory, "xt_blobs")


@pytest.fixture(scope="module")
def blobs():
    comp = pkg("compiler")
    with open(os.path.join(comp.RULES_DIR, "builtin_infotypes.yaml")) as f:
        builtin = yaml.safe_load(f)
    return {n: comp.compile_rules(comp.Rules(getattr(TC, n)(), builtin), text_exclusions=True) for n in GOOD}


@pytest.mark.parametrize("name", GOOD)
def test_text_exclusion_blobs_are_accepted(name, run, blobs):
    c = blobs[name]
    out = run(name, c.blob)
    assert out.startswith("ok "), out
    assert f"types={len(c.rules.type_names)} patterns={len(c.rules.patterns)} " in out


# ------------------------------------------------------------------------------------------ damage
def _dropped(name):
    def f(S):
        del S[name]
    f.__name__ = "dropped_" + name.replace(".", "_")
    return f


def _general_dropped(S):
    for k in ("var.xg_off", "var.xg_ids", "det.xgidx"):
        del S[k]


def _rule_cut(S):
    S["xt.rule"] = S["xt.rule"][:-1].copy()


def _desc_short(S):
    S["xt.desc"] = S["xt.desc"][:-8].copy()


def _cmap_short(S):
    S["xt.cmap"] = S["xt.cmap"][:-1].copy()


def _off_short(S):
    S["var.xt_off"] = S["var.xt_off"][:-1].copy()


def _off_nonzero(S):
    off = S["var.xt_off"].copy()
    off[0] = 1
    S["var.xt_off"] = off


def _off_descending(S):
    off = S["var.xt_off"].copy()
    k = int(np.flatnonzero(np.diff(off.astype(np.int64)) > 0)[1])
    off[k], off[k + 1] = off[k + 1], off[k]
    S["var.xt_off"] = off


def _ids_short(S):
    S["var.xt_ids"] = S["var.xt_ids"][:-1].copy()


def _rule_past_the_table(S):
    ids = S["var.xt_ids"].copy()
    ids[0] = len(S["xt.rule"]) // 4
    S["var.xt_ids"] = ids


def _rule_field(i, v):
    def f(S):
        r = S["xt.rule"].copy()
        h = int(np.flatnonzero(r.reshape(-1, 4)[:, 0] == 3)[0]) if i else 0      # (windows: of the hotword rule)
        r[4 * h + i] = v
        S["xt.rule"] = r
    return f


def _hotword_without_window(S):
    r = S["xt.rule"].copy()
    h = int(np.flatnonzero(r.reshape(-1, 4)[:, 0] == 3)[0])
    r[4 * h + 1] = r[4 * h + 2] = 0
    S["xt.rule"] = r


def _desc_field(i, v, rule=1):
    def f(S):
        d = S["xt.desc"].copy()
        d[8 * rule + i] = v(S, d[8 * rule:8 * rule + 8]) if callable(v) else v
        S["xt.desc"] = d
    return f


def _state_past_its_automaton(S):
    d, tr = S["xt.desc"], S["xt.trans"].copy()
    tr[int(d[8]) + 3] = int(d[8 + 7])                  # rule 1: an entry = its state count
    S["xt.trans"] = tr


def _class_past_its_automaton(S):
    d, cm = S["xt.desc"], S["xt.cmap"].copy()
    cm[int(d[8 + 2]) + 65] = int(d[8 + 3]) - 1         # rule 1: byte 'A' -> the end-of-text column
    S["xt.cmap"] = cm


NOT_ALL = "text exclusion sections are not all present"
SIZE = "xt.desc holds an automaton of impossible size"
DAMAGE = [(_dropped(s), NOT_ALL) for s in SECTIONS] + [
    (_general_dropped, "text exclusion sections without the general exclusion sections"),
    (_rule_cut, "xt.rule does not hold whole rules"),
    (_desc_short, "xt.desc does not hold one descriptor per rule"),
    (_cmap_short, "xt.cmap does not hold one class map per rule"),
    (_off_short, "var.xt_off does not hold V*T+1 offsets"),
    (_off_nonzero, "var.xt_off does not start at 0"),
    (_off_descending, "var.xt_off is not ascending"),
    (_ids_short, "var.xt_ids is shorter than its offsets"),
    (_rule_past_the_table, "var.xt_ids names a rule past the rule table"),
    (_rule_field(0, 4), "xt.rule holds an unknown kind"),
    (_rule_field(0, -1), "xt.rule holds an unknown kind"),
    (_rule_field(2, -5), "xt.rule holds a negative window"),
    (_hotword_without_window, "xt.rule holds a hotword rule without a window"),
    (_desc_field(3, 1), SIZE),
    (_desc_field(3, 257), SIZE),
    (_desc_field(7, 0), SIZE),
    (_desc_field(7, 1 << 15), SIZE),
    (_desc_field(0, lambda S, d: len(S["xt.trans"]) - int(d[7]) * int(d[3]) + 1), "xt.desc points past xt.trans"),
    (_desc_field(0, -2), "xt.desc points past xt.trans"),
    (_desc_field(1, lambda S, d: len(S["xt.flags"]) - int(d[7]) + 1), "xt.desc points past xt.flags"),
    (_desc_field(2, lambda S, d: len(S["xt.cmap"]) - 255), "xt.desc points past xt.cmap"),
    (_desc_field(4, lambda S, d: int(d[7])), "xt.desc holds a start state past its automaton"),
    (_state_past_its_automaton, "xt.trans holds a state past its automaton"),
    (_class_past_its_automaton, "xt.cmap holds a class past its automaton"),
]
IDS = ["%02d_%s" % (i, d.__name__.strip("_")) for i, (d, _) in enumerate(DAMAGE)]


@pytest.mark.parametrize("damage, message", DAMAGE, ids=IDS)
def test_damaged_text_exclusion_blob(damage, message, run, blobs):
    comp = pkg("compiler")
    S = comp.blob_sections(blobs["all_forms"].blob)
    assert comp._sections_to_blob(S) == blobs["all_forms"].blob       # the round trip itself changes nothing
    damage(S)
    assert run(damage.__name__.strip("_"), comp._sections_to_blob(S)) == "rejected: " + message
