#!/usr/bin/env python3
"""What the window re-scan costs under general and text exclusion rules, FULL against incremental
(PII_WINDOW_XG).

The config-3-shaped stream of bench.py --workload window (one new row of every conversation per call, the
whole stream resident in HBM, declared base and size).  Per configuration a fresh engine, N = 5 warm-up calls
(the windows fill) and --calls timed ones: the call time (HIP events around the whole call,
pii_last_timings [5]) and its median.  Configurations:

    plain            tests/excl_configs.py g1_no_rules (the custom types, no rule set of G1), incremental: the floor
    G1, G2, G3, hand tests/excl_configs.py and tests/text_excl_configs.py hand(); each in FULL (what an engine
                     enabled without the flag runs; --full-repeats times, for the spread of repeated runs) and
                     with the flag (G3 keeps its allow-list types: with PII_WINDOW_XF too)

The window bytes, output offsets and spans of every timed call of a flagged run are compared, on the GPU, with
those of the same rules' FULL run; a difference ends the tool.  One JSON line per run and a summary line per
rule set.  --profile re-runs the flagged configurations in a child process under
`rocprofv3 --kernel-trace --stats` (counters are not collected) and adds one line with the average time per
call of the window kernels, k_win_lik and k_win_xmark among them.

    python tools/window_xg_cost.py [--conversations 100000] [--calls 10] [--rules G1,G2,G3,hand]
                                   [--full-repeats 2] [--profile] [--out profiles/window_xg/xg_cost.jsonl]
"""
import argparse
import csv
import glob
import importlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KERNELS = ("k_win_cands", "k_win_halo", "k_win_plan", "k_win_lik", "k_win_xmark", "k_win_select", "k_win_alloc",
           "k_win_redact", "k_win_pos", "k_win_mask", "k_win_hash", "k_win_commit", "k_scan_lb")


def pkg(mod):
    return importlib.import_module("context-based-pii_amd." + mod)


def configs():
    XC, TC = importlib.import_module("excl_configs"), importlib.import_module("text_excl_configs")
    return XC, {"plain": XC.g1_no_rules, "G1": XC.g1, "G2": XC.g2, "G3": XC.g3, "hand": TC.hand}


class Stream:
    """the stream in HBM and the output buffers of one call"""

    def __init__(self, a):
        import torch
        bench = importlib.import_module("bench")
        synth = pkg("synth")
        self.C, self.N = a.conversations, 5
        self.U = self.N + a.calls
        C, U = self.C, self.U
        bank = synth.build_bank(16384, 16384, seed=synth.SEED)
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(0)
        self.meta = meta = synth.step_major(synth.corpus_meta(C, U, bank, seed=synth.SEED), bank, C, U)
        self.text, self.offs = bench.gpu_corpus(meta, bank, dev)
        self.slot = torch.from_numpy(meta.conv_slot.view(np.int32)).to(dev)
        self.role = torch.from_numpy(meta.role).to(dev)
        self.ts = torch.from_numpy(meta.ts_us).to(dev)
        self.step_bytes = [int(meta.offsets[(k + 1) * C] - meta.offsets[k * C]) for k in range(U)]
        self.out_cap = (self.N + 1) * max(self.step_bytes) + 64 * self.N * C
        self.span_cap = 8 * self.N * C
        self.d_out = torch.empty(self.out_cap, dtype=torch.uint8, device=dev)
        self.d_oo = torch.empty(C + 1, dtype=torch.int64, device=dev)
        self.d_sp = torch.empty(self.span_cap * 16, dtype=torch.uint8, device=dev)
        self.d_ctx = torch.empty(C, dtype=torch.int16, device=dev)

    def call(self, eng, q):
        C = self.C
        eng.rescan_window_device_ex(self.text.data_ptr(), self.offs.data_ptr() + 8 * q * C, C, int(self.meta.offsets[q * C]),
                                    self.step_bytes[q], self.slot.data_ptr() + 4 * q * C, self.role.data_ptr() + q * C,
                                    self.ts.data_ptr() + 8 * q * C, self.d_out.data_ptr(), self.out_cap, self.d_oo.data_ptr(),
                                    self.d_sp.data_ptr(), self.span_cap, self.d_ctx.data_ptr())
        ob, ns, flags = eng.sync()
        assert flags == 0, flags
        return ob, ns


def enable(eng, rules, full, flagged):
    if full:
        eng.window_enable(5, 8192, full=True)
    else:
        eng.window_enable(5, 8192, incremental_transforms=flagged and rules == "G3", incremental_exclusions=flagged)


def run(a, out):
    import torch
    comp, E = pkg("compiler"), pkg("engine")
    XC, make = configs()
    S = Stream(a)

    def one(blob, rules, full, flagged, keep):
        """a fresh engine over the stream -> (per-call ms, last bytes out, last findings, mode, kept results)"""
        eng = E.Engine(blob, device=0, n_conv_slots=S.C)
        enable(eng, rules, full, flagged)
        torch.cuda.synchronize()
        ms, ob, ns, kept = [], 0, 0, []
        for q in range(S.U):
            ob, ns = S.call(eng, q)
            if q >= S.N:
                ms.append(eng.timings()[5])
                if keep:
                    kept.append((S.d_out[:ob].clone(), S.d_oo.clone(), S.d_sp[:ns * 16].clone()))
        mode = eng.window_mode()
        eng.close()
        return ms, int(ob), int(ns), mode, kept

    def line(rules, run_name, ms, ob, ns, mode):
        ln = {"rules": rules, "run": run_name, "mode": mode, "rows_per_call": S.C, "new_bytes_per_call": S.step_bytes[-1],
              "window_bytes_out": ob, "window_findings": ns, "call_ms": [round(x, 4) for x in ms],
              "call_ms_median": round(statistics.median(ms), 4)}
        print(json.dumps(ln), flush=True)
        out.append(ln)
        return ln["call_ms_median"]

    with tempfile.TemporaryDirectory() as d:
        floor = None
        for rules in ["plain"] + [r for r in a.rules.split(",") if r]:
            blob = comp.compile_default(XC.write(d, rules, make[rules]())).blob
            if rules == "plain":
                ms, ob, ns, mode, _ = one(blob, rules, False, False, False)
                assert mode == "incremental"
                floor = line(rules, "incremental", ms, ob, ns, mode)
                continue
            fulls, ref = [], None
            for k in range(a.full_repeats):
                ms, ob, ns, mode, kept = one(blob, rules, True, False, k == 0)
                assert mode == "full"
                fulls.append(line(rules, f"full_{k}", ms, ob, ns, mode))
                ref = kept if k == 0 else ref
            ms, ob, ns, mode, kept = one(blob, rules, False, True, True)
            assert mode == "incremental"
            flagged = line(rules, "flagged", ms, ob, ns, mode)
            for q, (x, y) in enumerate(zip(ref, kept)):
                if not all(p.shape == r.shape and torch.equal(p, r) for p, r in zip(x, y)):
                    raise SystemExit(f"{rules}: timed call {q}: the flagged run's output differs from the FULL run's")
            ln = {"rules": rules, "summary": True, "full_ms": fulls, "full_spread_ms": round(max(fulls) - min(fulls), 4),
                  "flagged_ms": flagged, "full_minus_flagged_ms": round(min(fulls) - flagged, 4),
                  "flagged_over_floor": round(flagged / floor, 3), "outputs_equal_calls": len(kept)}
            print(json.dumps(ln), flush=True)
            out.append(ln)


def profile(a, out):
    """the flagged configurations in a child under rocprofv3: average time per call of the window kernels"""
    for rules in [r for r in a.rules.split(",") if r]:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                   os.path.abspath(__file__), "--conversations", str(a.conversations), "--calls", str(a.calls),
                   "--rules", rules, "--flagged-only"]
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
            files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            if not files:
                raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
            per = {}
            with open(files[0]) as f:
                for r in csv.DictReader(f):
                    short = r["Name"].replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0]
                    if short.split("<")[0] in KERNELS:
                        per[short] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2)}
        ln = {"rocprofv3_kernel_stats": True, "rules": rules, "run": "flagged", "rows_per_call": a.conversations,
              "kernels": dict(sorted(per.items()))}
        print(json.dumps(ln), flush=True)
        out.append(ln)


def flagged_only(a):
    """the child of --profile: one rule set, flagged, nothing kept or compared"""
    comp, E = pkg("compiler"), pkg("engine")
    XC, make = configs()
    S = Stream(a)
    with tempfile.TemporaryDirectory() as d:
        blob = comp.compile_default(XC.write(d, a.rules, make[a.rules]())).blob
    eng = E.Engine(blob, device=0, n_conv_slots=S.C)
    enable(eng, a.rules, False, True)
    for q in range(S.U):
        S.call(eng, q)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conversations", type=int, default=100_000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rules", default="G1,G2,G3,hand")
    ap.add_argument("--full-repeats", type=int, default=2)
    ap.add_argument("--profile", action="store_true", help="only the rocprofv3 child runs (kernel times)")
    ap.add_argument("--flagged-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    if a.flagged_only:
        return flagged_only(a)
    out = []
    (profile if a.profile else run)(a, out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in out:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
