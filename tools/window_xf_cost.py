#!/usr/bin/env python3
"""What the window re-scan costs under mask, keep, hash and FPE transformations, FULL against incremental
(PII_WINDOW_XF).

The config-3-shaped stream of bench.py --workload window (one new row of every conversation per call, the
whole stream resident in HBM, declared base and size).  Per configuration a fresh engine, N = 5 warm-up calls
(the windows fill) and --calls timed ones: the call time (HIP events around the whole call,
pii_last_timings [5]) and its median.  Configurations:

    shipped      the shipped rules, incremental: the floor
    A, B, H, HC  tests/xform_configs.py and tests/xform_hash_ref.py; each in FULL (what an engine enabled
                 without the flag runs; --full-repeats times, for the spread of repeated runs) and with the flag
    F, FC        tests/xform_fpe_ref.py (crypto_replace_ffx_fpe_config), likewise; asked for with --rules

The window bytes, output offsets and spans of every timed call of a flagged run are compared, on the GPU, with
those of the same rules' FULL run; a difference ends the tool.  One JSON line per run and a summary line per
rule set.  --profile re-runs the flagged configurations in a child process under
`rocprofv3 --kernel-trace --stats` (counters are not collected) and adds one line with the average time per
call of the window kernels, k_win_pos, k_win_mask, k_win_hash and k_win_fpe among them.

    python tools/window_xf_cost.py [--conversations 100000] [--calls 10] [--rules A,B,H,HC] [--full-repeats 2]
                                   [--profile] [--out profiles/window_xf/xf_cost.jsonl]
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

KERNELS = ("k_win_cands", "k_win_halo", "k_win_plan", "k_win_select", "k_win_alloc", "k_win_redact", "k_win_pos",
           "k_win_mask", "k_win_hash", "k_win_fpe", "k_win_commit", "k_scan_lb")


def pkg(mod):
    return importlib.import_module("context-based-pii_amd." + mod)


def blocks():
    X, HR = importlib.import_module("xform_configs"), importlib.import_module("xform_hash_ref")
    FR = importlib.import_module("xform_fpe_ref")
    return X, {"shipped": None, "A": X.A, "B": X.B, "H": HR.H, "HC": HR.HC, "F": FR.F, "FC": FR.FC}


def run(a, out):
    import torch
    bench = importlib.import_module("bench")
    comp, E, synth = pkg("compiler"), pkg("engine"), pkg("synth")
    X, B = blocks()
    C, N = a.conversations, 5
    U = N + a.calls
    bank = synth.build_bank(16384, 16384, seed=synth.SEED)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    meta = synth.step_major(synth.corpus_meta(C, U, bank, seed=synth.SEED), bank, C, U)
    text, offs = bench.gpu_corpus(meta, bank, dev)
    slot = torch.from_numpy(meta.conv_slot.view(np.int32)).to(dev)
    role = torch.from_numpy(meta.role).to(dev)
    ts = torch.from_numpy(meta.ts_us).to(dev)
    step_bytes = [int(meta.offsets[(k + 1) * C] - meta.offsets[k * C]) for k in range(U)]
    out_cap = (N + 1) * max(step_bytes) + 64 * N * C
    span_cap = 8 * N * C
    d_out = torch.empty(out_cap, dtype=torch.uint8, device=dev)
    d_oo = torch.empty(C + 1, dtype=torch.int64, device=dev)
    d_sp = torch.empty(span_cap * 16, dtype=torch.uint8, device=dev)
    d_ctx = torch.empty(C, dtype=torch.int16, device=dev)

    def one(blob, full, xf, keep):
        """a fresh engine over the stream -> (per-call ms, last bytes out, last findings, mode, kept results)"""
        eng = E.Engine(blob, device=0, n_conv_slots=C)
        eng.window_enable(N, 8192, full=full, incremental_transforms=xf)
        torch.cuda.synchronize()
        ms, ob, ns, kept = [], 0, 0, []
        for q in range(U):
            eng.rescan_window_device_ex(text.data_ptr(), offs.data_ptr() + 8 * q * C, C, int(meta.offsets[q * C]),
                                        step_bytes[q], slot.data_ptr() + 4 * q * C, role.data_ptr() + q * C,
                                        ts.data_ptr() + 8 * q * C, d_out.data_ptr(), out_cap, d_oo.data_ptr(),
                                        d_sp.data_ptr(), span_cap, d_ctx.data_ptr())
            ob, ns, flags = eng.sync()
            assert flags == 0, flags
            if q >= N:
                ms.append(eng.timings()[5])
                if keep:
                    kept.append((d_out[:ob].clone(), d_oo.clone(), d_sp[:ns * 16].clone()))
        mode = eng.window_mode()
        eng.close()
        return ms, int(ob), int(ns), mode, kept

    def line(rules, run_name, ms, ob, ns, mode):
        ln = {"rules": rules, "run": run_name, "mode": mode, "rows_per_call": C, "new_bytes_per_call": step_bytes[-1],
              "window_bytes_out": ob, "window_findings": ns, "call_ms": [round(x, 4) for x in ms],
              "call_ms_median": round(statistics.median(ms), 4)}
        print(json.dumps(ln), flush=True)
        out.append(ln)
        return ln["call_ms_median"]

    with tempfile.TemporaryDirectory() as d:
        floor = None
        for rules in ["shipped"] + [r for r in a.rules.split(",") if r]:
            blob = comp.compile_default(X.write(d, rules, X.with_block(B[rules]))).blob
            if rules == "shipped":
                ms, ob, ns, mode, _ = one(blob, False, False, False)
                floor = line(rules, "incremental", ms, ob, ns, mode)
                continue
            fulls, ref = [], None
            for k in range(a.full_repeats):
                ms, ob, ns, mode, kept = one(blob, True, False, k == 0)
                assert mode == "full"
                fulls.append(line(rules, f"full_{k}", ms, ob, ns, mode))
                ref = kept if k == 0 else ref
            ms, ob, ns, mode, kept = one(blob, False, True, True)
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
    import torch
    bench = importlib.import_module("bench")
    comp, E, synth = pkg("compiler"), pkg("engine"), pkg("synth")
    X, B = blocks()
    C, N = a.conversations, 5
    U = N + a.calls
    bank = synth.build_bank(16384, 16384, seed=synth.SEED)
    dev = torch.device("cuda", 0)
    meta = synth.step_major(synth.corpus_meta(C, U, bank, seed=synth.SEED), bank, C, U)
    text, offs = bench.gpu_corpus(meta, bank, dev)
    slot = torch.from_numpy(meta.conv_slot.view(np.int32)).to(dev)
    role = torch.from_numpy(meta.role).to(dev)
    ts = torch.from_numpy(meta.ts_us).to(dev)
    step_bytes = [int(meta.offsets[(k + 1) * C] - meta.offsets[k * C]) for k in range(U)]
    out_cap, span_cap = (N + 1) * max(step_bytes) + 64 * N * C, 8 * N * C
    d_out = torch.empty(out_cap, dtype=torch.uint8, device=dev)
    d_oo = torch.empty(C + 1, dtype=torch.int64, device=dev)
    d_sp = torch.empty(span_cap * 16, dtype=torch.uint8, device=dev)
    d_ctx = torch.empty(C, dtype=torch.int16, device=dev)
    with tempfile.TemporaryDirectory() as d:
        blob = comp.compile_default(X.write(d, a.rules, X.with_block(B[a.rules]))).blob
    eng = E.Engine(blob, device=0, n_conv_slots=C)
    eng.window_enable(N, 8192, incremental_transforms=True)
    for q in range(U):
        eng.rescan_window_device_ex(text.data_ptr(), offs.data_ptr() + 8 * q * C, C, int(meta.offsets[q * C]),
                                    step_bytes[q], slot.data_ptr() + 4 * q * C, role.data_ptr() + q * C,
                                    ts.data_ptr() + 8 * q * C, d_out.data_ptr(), out_cap, d_oo.data_ptr(),
                                    d_sp.data_ptr(), span_cap, d_ctx.data_ptr())
        assert eng.sync()[2] == 0
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conversations", type=int, default=100_000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rules", default="A,B,H,HC")
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
