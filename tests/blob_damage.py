"""Rule blobs damaged one section at a time, and what pii_engine_create makes of each: shared by the GPU
test of the hash sections (test_gpu_hash), the C ABI test (test_abi) and the stand-alone run of the host
rule preparation under the sanitizers (test_rules_host)."""
import inspect

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


HASH_DAMAGE = [_hash_mid_dropped, _hash_key_dropped, _key_index_out_of_range, _mid_cut_short, _key_table_short,
               _placeholder_short]
# damage -> the message of the first defect the host rule preparation meets
MESSAGES = {**{d: XF_MALFORMED for d in HASH_DAMAGE},
            _first_pre_past_its_automaton: "det.first_pre names a state past its automaton",
            _first_pre_short: "det.first_pre is too short"}
ALL_DAMAGE = list(MESSAGES)


def damage_id(f):
    return f.__name__.strip("_")


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
    S = comp.blob_sections(compiled.blob)
    assert comp._sections_to_blob(S) == compiled.blob              # the round trip itself changes nothing
    if len(inspect.signature(damage).parameters) == 2:
        damage(S, compiled.rules.type_names)
    else:
        damage(S)
    return comp._sections_to_blob(S)
