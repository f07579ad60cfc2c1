#!/usr/bin/env python3
"""What the text exclusion rules (k_excl_text) cost ("Text exclusion rules").

The synthetic device batch of tools/excl_cost.py (conversation-major rows from the synth bank), run through
three engines: the all-forms allow-list of the text exclusion tests (tests/text_excl_configs.py all_forms:
regex PARTIAL / FULL / INVERSE, a dictionary and an exclude_by_hotword rule beside the shipped
exclude_info_types rule -- general, k_exclude's phases and k_excl_text run), the same config with the text
rules removed (the shipped rules: streaming, neither runs), and text_only (the text rules without any
exclude_info_types rule: k_excl_text alone).  Per engine the call time (HIP events around the whole call,
pii_last_timings [5]) of --calls calls after one warm-up call, and their median.  One JSON line per engine
and a summary line.  The kernels' own times come from a `rocprofv3 --kernel-trace --stats` run of this
script (--configs all_forms), with k_select's time in the same run as the yardstick.

--share N (no GPU): over the first N rows of the batch, the share of matched pairs (a FIRST run that
matched: what k_excl_text walks) whose (variant, type) has a rule list -- the kernel's time scales with it --
counted with the tables' Python restatement (tests/tablesim.py).

    python tools/text_excl_cost.py [--conversations 30000] [--rows-per-conversation 20] [--calls 5]
                                   [--configs no_text_rules,text_only,all_forms] [--share 0]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def pkg(mod):
    return importlib.import_module("context-based-pii_amd." + mod)


def configs():
    import text_excl_configs as TC
    import text_excl_ref as TR
    return {"no_text_rules": lambda: TR.without_text_rules(TC.all_forms()), "text_only": TC.text_only,
            "all_forms": TC.all_forms}


def compile_cfg(name):
    import text_excl_configs as TC
    with tempfile.TemporaryDirectory() as d:
        return pkg("compiler").compile_default(TC.write(d, name, configs()[name]()))


def share(corp, n_rows):
    """matched pairs of the first n_rows rows (no context: the rule sets are in every variant) and those
    whose type has a text rule list"""
    from tablesim import TableSim
    c = compile_cfg("all_forms")
    sim = TableSim(c)
    S = c.sections
    T = int(S["meta"][2])
    has = [int(S["var.xt_off"][t + 1]) > int(S["var.xt_off"][t]) for t in range(T)]
    matched = listed = 0
    for i in range(n_rows):
        text = corp.data[int(corp.offsets[i]):int(corp.offsets[i + 1])].tobytes()
        for pos, sd, _sk in sim.scan(text, agent=False):
            a = sim.d_accept(text, pos, sd)
            for k in range(int(sim.d_off[a]), int(sim.d_off[a + 1])):
                p = int(sim.d_ids[k])
                if sim.first_run(p, text, pos) >= 0:
                    matched += 1
                    listed += has[int(sim.det_type[p])]
    print(json.dumps({"rows": n_rows, "matched_pairs": matched, "with_a_rule_list": listed,
                      "share": round(listed / max(1, matched), 4)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conversations", type=int, default=30000)
    ap.add_argument("--rows-per-conversation", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--configs", default="no_text_rules,text_only,all_forms")
    ap.add_argument("--share", type=int, default=0)
    a = ap.parse_args()
    comp, E, synth = pkg("compiler"), pkg("engine"), pkg("synth")
    corp = synth.make_corpus(a.conversations, a.rows_per_conversation, synth.build_bank())
    if a.share:
        share(corp, min(a.share, corp.n))
        return
    import torch
    n, total = corp.n, int(corp.offsets[-1])
    dev = torch.device("cuda:0")
    d_text = torch.from_numpy(np.concatenate([corp.data, np.zeros(64, np.uint8)])).to(dev)
    d_offs = torch.from_numpy(np.ascontiguousarray(corp.offsets).view(np.int64)).to(dev)
    d_slot = torch.from_numpy(np.ascontiguousarray(corp.conv_slot, dtype=np.uint32).view(np.int32)).to(dev)
    d_role = torch.from_numpy(np.ascontiguousarray(corp.role, dtype=np.uint8)).to(dev)
    d_ts = torch.from_numpy(np.ascontiguousarray(corp.ts_us, dtype=np.int64)).to(dev)
    out_cap, span_cap = total + 64 * n, n
    d_out = torch.empty(out_cap + 32, dtype=torch.uint8, device=dev)
    d_oo = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_sp = torch.empty(span_cap * 16, dtype=torch.uint8, device=dev)
    d_ctx = torch.empty(n, dtype=torch.int16, device=dev)
    med = {}
    for name in a.configs.split(","):
        eng = E.Engine(compile_cfg(name).blob, device=0, n_conv_slots=a.conversations)
        ms = []
        for _ in range(1 + a.calls):
            eng.scan_redact_device(d_text.data_ptr(), d_offs.data_ptr(), n, d_slot.data_ptr(), d_role.data_ptr(),
                                   d_ts.data_ptr(), d_out.data_ptr(), out_cap, d_oo.data_ptr(), d_sp.data_ptr(),
                                   span_cap, d_ctx.data_ptr())
            ob, ns, flags = eng.sync()
            assert flags == 0, flags
            ms.append(eng.timings()[5])
        st = eng.stats(gate=True)
        mode, occ = eng.exclusion_mode(), eng.exclusion_occurrences()
        eng.close()
        med[name] = statistics.median(ms[1:])
        print(json.dumps({"config": name, "exclusion_mode": mode, "rows": n, "bytes_in": total, "bytes_out": ob,
                          "findings": int(ns), "pairs": st["pairs"], "occurrences": occ, "lane_bytes": st["lane_bytes"],
                          "reruns_last_call": st["reruns"], "call_ms": [round(x, 4) for x in ms[1:]],
                          "call_ms_median": round(med[name], 4)}), flush=True)
    if "no_text_rules" in med and len(med) > 1:
        base = med["no_text_rules"]
        print(json.dumps({"bytes_in": total, **{k + "_minus_no_text_rules_ms": round(v - base, 4)
                                                for k, v in med.items() if k != "no_text_rules"},
                          **{k + "_share_of_call": round((v - base) / base, 4)
                             for k, v in med.items() if k != "no_text_rules"}}))


if __name__ == "__main__":
    main()
