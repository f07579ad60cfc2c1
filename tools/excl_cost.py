#!/usr/bin/env python3
"""What the general exclusion pass (k_exclude) costs ("General exclusion rules").

The synthetic device batch of tools/xf_hash_cost.py (conversation-major rows from the synth bank), run
through two engines: the allow-list config G1 of the exclusion tests (tests/excl_configs.py: four custom
regex types, PARTIAL_MATCH and FULL_MATCH rules over them -- general, so k_exclude runs) and the same
config with those rule sets removed and the custom types kept (streaming, no k_exclude).  Per engine the
call time (HIP events around the whole call, pii_last_timings [5]) of --calls calls after one warm-up
call, and their median; the difference of the medians is the pass.  One JSON line per engine and a summary
line.  The kernels' own times come from a `rocprofv3 --kernel-trace --stats` run of this script
(--configs g1), with k_select's time in the same run as the yardstick.

    python tools/excl_cost.py [--conversations 30000] [--rows-per-conversation 20] [--calls 5] [--configs g1_no_rules,g1]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conversations", type=int, default=30000)
    ap.add_argument("--rows-per-conversation", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--configs", default="g1_no_rules,g1")
    a = ap.parse_args()
    import torch
    import excl_configs as XC
    comp, E, synth = pkg("compiler"), pkg("engine"), pkg("synth")
    corp = synth.make_corpus(a.conversations, a.rows_per_conversation, synth.build_bank())
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
    configs = {"g1_no_rules": XC.g1_no_rules, "g1": XC.g1}
    med = {}
    for name in a.configs.split(","):
        with tempfile.TemporaryDirectory() as d:
            blob = comp.compile_default(XC.write(d, name, configs[name]())).blob
        eng = E.Engine(blob, device=0, n_conv_slots=a.conversations)
        ms = []
        for _ in range(1 + a.calls):
            eng.scan_redact_device(d_text.data_ptr(), d_offs.data_ptr(), n, d_slot.data_ptr(), d_role.data_ptr(),
                                   d_ts.data_ptr(), d_out.data_ptr(), out_cap, d_oo.data_ptr(), d_sp.data_ptr(),
                                   span_cap, d_ctx.data_ptr())
            ob, ns, flags = eng.sync()
            assert flags == 0, flags
            ms.append(eng.timings()[5])
        st = eng.stats(gate=True)
        mode = eng.exclusion_mode()
        eng.close()
        med[name] = statistics.median(ms[1:])
        print(json.dumps({"config": name, "exclusion_mode": mode, "rows": n, "bytes_in": total, "bytes_out": ob,
                          "findings": int(ns), "pairs": st["pairs"], "lane_bytes": st["lane_bytes"],
                          "reruns_last_call": st["reruns"], "call_ms": [round(x, 4) for x in ms[1:]],
                          "call_ms_median": round(med[name], 4)}), flush=True)
    if len(med) == 2:
        print(json.dumps({"bytes_in": total, "k_exclude_ms": round(med["g1"] - med["g1_no_rules"], 4),
                          "share_of_call": round((med["g1"] - med["g1_no_rules"]) / med["g1_no_rules"], 4)}))


if __name__ == "__main__":
    main()
