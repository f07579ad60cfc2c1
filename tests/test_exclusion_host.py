"""The host rule preparation (csrc/pii_rules_host.h) over general exclusion blobs, on its own: the
stand-alone program of test_rules_host (tests/rules_host_main.cpp, built with the host compiler under the
address and undefined-behaviour sanitizers) accepts the G1 and G2 blobs and rejects, each with its own
message, blobs whose general exclusion sections are damaged one at a time."""
import os

import numpy as np
import pytest
import yaml

import excl_configs as XC
import rules_host_runner
from conftest import pkg

SECTIONS = ("var.xg_off", "var.xg_ids", "det.xgidx")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    return rules_host_runner.runner(tmp_path_factory, "excl_blobs")


@pytest.fixture(scope="module")
def blobs():
    comp = pkg("compiler")
    with open(os.path.join(comp.RULES_DIR, "builtin_infotypes.yaml")) as f:
        builtin = yaml.safe_load(f)
    return {n: comp.compile_rules(comp.Rules(XC.CONFIGS[n](), builtin)) for n in ("G1", "G2")}


@pytest.mark.parametrize("name", ["G1", "G2"])
def test_general_blobs_are_accepted(name, run, blobs):
    """(G2 before general exclusion rules: "rejected: too many excluder patterns")"""
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


def _xg_off_short(S):
    S["var.xg_off"] = S["var.xg_off"][:-1].copy()


def _xgidx_short(S):
    S["det.xgidx"] = S["det.xgidx"][:-1].copy()


def _xg_ids_short(S):
    S["var.xg_ids"] = S["var.xg_ids"][:int(S["var.xg_off"][-1]) - 1].copy()


def _xg_off_descending(S):
    off = S["var.xg_off"].copy()
    k = int(np.flatnonzero(np.diff(off.astype(np.int64)) > 0)[1])      # (not key 0: off[0] stays 0)
    off[k], off[k + 1] = off[k + 1], off[k]
    S["var.xg_off"] = off


def _type_past_the_table(S):
    ids = S["var.xg_ids"].copy()
    ids[0] = (int(ids[0]) & 0x8000) | int(S["meta"][2])             # id = T, the matching bit kept
    S["var.xg_ids"] = ids


def _index_past_the_limit(S):
    idx = S["det.xgidx"].copy()
    idx[int(np.flatnonzero(idx != 0xFF)[0])] = pkg("compiler").NX_MAX
    S["det.xgidx"] = idx


def _streaming_slot_beside(S):
    ex = S["det.exidx"].copy()
    ex[0] = 0
    S["det.exidx"] = ex


def _streaming_list_beside(S):
    S["var.excl_off"] = S["var.xg_off"].copy()
    S["var.excl_ids"] = (S["var.xg_ids"] & 0x7FFF).astype(np.uint16)


NOT_ALL = "general exclusion sections are not all present"
BESIDE = "general exclusion sections beside streaming exclusion lists"
DAMAGE = [(_dropped(s), NOT_ALL) for s in SECTIONS] + [
    (_xg_off_short, "var.xg_off does not hold V*T+1 offsets"),
    (_xgidx_short, "det.xgidx does not hold one index per pattern"),
    (_xg_ids_short, "var.xg_ids is shorter than its offsets"),
    (_xg_off_descending, "var.xg_off is not ascending"),
    (_type_past_the_table, "var.xg_ids names a type past the type table"),
    (_index_past_the_limit, "det.xgidx holds an index past the limit"),
    (_streaming_slot_beside, BESIDE),
    (_streaming_list_beside, BESIDE),
]


@pytest.mark.parametrize("damage, message", DAMAGE, ids=[d.__name__.strip("_") for d, _ in DAMAGE])
def test_damaged_general_blob(damage, message, run, blobs):
    comp = pkg("compiler")
    S = comp.blob_sections(blobs["G1"].blob)
    assert comp._sections_to_blob(S) == blobs["G1"].blob              # the round trip itself changes nothing
    damage(S)
    assert run(damage.__name__.strip("_"), comp._sections_to_blob(S)) == "rejected: " + message
