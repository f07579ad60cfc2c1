"""Rule blobs damaged one section at a time, and what pii_engine_create makes of each: shared by the GPU
test of the hash sections (test_gpu_hash), the C ABI test (test_abi) and the stand-alone run of the host
rule preparation under the sanitizers (test_rules_host).  HASH_DAMAGE: the hash sections; CORE_DAMAGE: the
required sections (cut to half, one value out of range, another dtype code), each with its own message."""
import functools
import inspect
import os
import tempfile

import numpy as np

import xform_configs as X
import xform_hash_ref as HR
from conftest import pkg

XF_MALFORMED = "transformation tables malformed"


def _hash_mid_dropped(S):
    del S["xf.hash_mid"]


def _hash_key_dropped(S):
    del S["xf.hash_key"]


def _key_index_out_of_range(S, names):
    S["xf.hash_key"] = S["xf.hash_key"].copy()
    S["xf.hash_key"][names.index("PHONE_NUMBER")] = 2                # two keys: 0 and 1


def _mid_cut_short(S):
    S["xf.hash_mid"] = S["xf.hash_mid"][:24].copy()


def _key_table_short(S):
    S["xf.hash_key"] = S["xf.hash_key"][:-1].copy()


def _placeholder_short(S, names):
    off = S["xf.repl_off"].copy()
    t = names.index("PHONE_NUMBER")
    off[t + 1:] -= 1                                                   # 43 bytes for one hash type
    S["xf.repl_off"] = off


def _first_pre_past_its_automaton(S):
    pre = S["det.first_pre"].copy()
    pre[0] = S["det.first_desc"].reshape(-1, 8)[0, 7]                  # n_states: one past the last state
    S["det.first_pre"] = pre


def _first_pre_short(S):
    S["det.first_pre"] = S["det.first_pre"][:-1].copy()


# ------------------------------------------------------------------------------ the required sections
def _halved(name):
    def f(S):
        S[name] = S[name][:len(S[name]) // 2].copy()
    f.__name__ = "halved_" + name.replace(".", "_")
    return f


def _poke(name, index, value):
    """one entry of a section overwritten; index and value may be computed from the sections"""
    def f(S):
        a = S[name].copy()
        a[index(S) if callable(index) else index] = value(S) if callable(value) else value
        S[name] = a
    return f


def _named(name, f, on=None):
    f.__name__ = name
    if on:
        f.on = on
    return f


def _retyped_det_lik(S):
    S["det.lik"] = S["det.lik"].view(np.int8)                          # the same bytes under another dtype code


PER_ENTRY = " does not hold one entry per state and class"
PAST_SETS = " names an accept set past the accept sets"
SHORT = " is shorter than its offsets"
# every required section but types.names cut to half its length -> what the preparation says of it
HALVED = {
    "meta": "meta does not hold 15 values",
    "scan.cmap2": "scan.cmap2 does not hold one class pair per byte",
    "scan.d.trans": "scan.d.trans" + PER_ENTRY,
    "scan.d.accid": "scan.d.accid" + PER_ENTRY,
    "scan.d.acc_off": "scan.d.accid" + PAST_SETS,                      # (half the sets: the table names the others)
    "scan.d.acc_ids": "scan.d.acc_ids" + SHORT,
    "scan.k.trans": "scan.k.trans" + PER_ENTRY,
    "scan.k.accid": "scan.k.accid" + PER_ENTRY,
    "scan.k.acc_off": "scan.k.accid" + PAST_SETS,
    "scan.k.acc_ids": "scan.k.acc_ids" + SHORT,
    "det.type": "det.type does not hold one type per pattern",
    "det.validator": "det.validator does not hold one validator per pattern",
    "det.lik": "det.lik does not hold one likelihood per pattern",
    "det.exidx": "det.exidx does not hold one excluder slot per pattern",
    "det.first_desc": "det.first_desc does not hold one descriptor per pattern",
    "hot.rule": "hot.rule does not hold one entry per hotword rule",
    "hot.dfa_desc": "hot.dfa_desc does not hold one descriptor per hotword rule",
    "pool.trans": "det.first_desc points past pool.trans",
    "pool.flags": "det.first_desc points past pool.flags",
    "pool.cmap": "det.first_desc points past pool.cmap",
    "var.enabled": "var.enabled does not hold one flag per variant and type",
    "var.minlik": "var.minlik does not hold one likelihood per variant",
    "var.rule_off": "var.rule_off does not hold V*T+1 offsets",
    "var.rule_ids": "var.rule_ids" + SHORT,
    "var.excl_off": "var.excl_off does not hold V*T+1 offsets",
    "var.excl_ids": "var.excl_ids" + SHORT,
    "kw.type": "kw.type does not hold one type per context group",
    "kw.always": "kw.always does not hold one flag per context group",
}


def _desc0(S, i):
    return int(S["det.first_desc"][i])                                 # pattern 0's descriptor, word i


# single values (meta: P, G, T, V, SD, CD, the D start state, ...)
CORE_MESSAGES = {
    **{_halved(s): m for s, m in HALVED.items()},
    _named("d_trans_past_SD",
           _poke("scan.d.trans", 5, lambda S: (int(S["scan.d.trans"][5]) & 0x8000) | int(S["meta"][4]))):
        "scan.d.trans holds a state past its automaton",
    _named("d_accid_past_the_sets", _poke("scan.d.accid", 5, lambda S: len(S["scan.d.acc_off"]) - 1)):
        "scan.d.accid" + PAST_SETS,
    _named("first_desc_past_pool_trans", _poke("det.first_desc", 0, lambda S: len(S["pool.trans"]))):
        "det.first_desc points past pool.trans",
    _named("pool_state_past_its_automaton", _poke("pool.trans", lambda S: _desc0(S, 0) + 3, lambda S: _desc0(S, 7))):
        "pool.trans holds a state past its automaton",
    _named("rule_off_2_to_20", _poke("var.rule_off", 1, 1 << 20)): "var.rule_off is not ascending",
    _named("d_start_past_SD", _poke("meta", 6, lambda S: int(S["meta"][4]))): "meta names a D start state past its automaton",
    _named("negative_pattern_count", _poke("meta", 0, -5)): "meta holds a dimension out of range",
    # byte 'A' -> the end-of-text column, in pattern 0's class map and in the D half of the SCAN class map
    _named("pool_class_past_its_automaton", _poke("pool.cmap", lambda S: _desc0(S, 2) + 65, lambda S: _desc0(S, 3) - 1)):
        "pool.cmap holds a class past its automaton",
    _named("scan_class_past_its_automaton",
           _poke("scan.cmap2", 65, lambda S: (int(S["scan.cmap2"][65]) & 0xFF00) | (int(S["meta"][5]) - 1))):
        "scan.cmap2 holds a class past its automaton",
    _named("group_trans_past_its_group", on="config5",
           f=_poke("scan.g1.trans", 5, lambda S: (int(S["scan.g1.trans"][5]) & 0x8000) | int(S["scan.groups"][0]))):
        "scan.g1.trans holds a state past its automaton",
    _retyped_det_lik: "det.lik does not hold u8 values",
}
CORE_DAMAGE = list(CORE_MESSAGES)

HASH_DAMAGE = [_hash_mid_dropped, _hash_key_dropped, _key_index_out_of_range, _mid_cut_short, _key_table_short,
               _placeholder_short]
# damage -> the message of the first defect the host rule preparation meets
MESSAGES = {**{d: XF_MALFORMED for d in HASH_DAMAGE},
            _first_pre_past_its_automaton: "det.first_pre names a state past its automaton",
            _first_pre_short: "det.first_pre is too short",
            **CORE_MESSAGES}
ALL_DAMAGE = list(MESSAGES)


def damage_id(f):
    return f.__name__.strip("_")


@functools.lru_cache(maxsize=None)
def config5_compiled():
    """rulegen.Config5 compiled (several SCAN groups; about a minute, so once per run)"""
    comp = pkg("compiler")
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "config5.json")
        pkg("rulegen").Config5().save(path)
        return comp.compile_rules(comp.Rules.load(path))


def hash_config_compiled():
    """the H config of xform_hash_ref (two keys, four hash types), compiled as test_hash_compile does"""
    import os
    import yaml
    comp = pkg("compiler")
    with open(os.path.join(comp.RULES_DIR, "builtin_infotypes.yaml")) as f:
        builtin = yaml.safe_load(f)
    return comp.compile_rules(comp.Rules(X.with_block(HR.H), builtin))


def damaged_blob(compiled, damage) -> bytes:
    comp = pkg("compiler")
    if getattr(damage, "on", None) == "config5":                   # (a damage that needs SCAN groups >= 1)
        compiled = config5_compiled()
    S = comp.blob_sections(compiled.blob)
    assert comp._sections_to_blob(S) == compiled.blob              # the round trip itself changes nothing
    if len(inspect.signature(damage).parameters) == 2:
        damage(S, compiled.rules.type_names)
    else:
        damage(S)
    return comp._sections_to_blob(S)
