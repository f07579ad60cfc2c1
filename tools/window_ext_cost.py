#!/usr/bin/env python3
"""What external candidates cost on the window re-scan ("External candidates on the window path").

The config-3-shaped stream of bench.py --workload window (one new row of every conversation per call, the
whole stream resident in HBM, declared base and size: no device-to-host read before a launch), with k
candidates per row, each up to 8 bytes long and spread evenly over its row (rows shorter than that get what
fits).  Per configuration a fresh engine, N warm-up calls (the windows fill) and --calls timed ones: the call
time (HIP events around the whole call, pii_last_timings [5]) and its median.  Configurations:

    0    the plain pii_rescan_window_device_ex on an engine that has never seen a candidate: the baseline
    0x   pii_rescan_window_device_ext with every list empty: the merge launches and the XR kernels alone
    1, 4 that many candidates per row

One JSON line per configuration and a summary line.  --profile re-runs the configurations in a child
process under `rocprofv3 --kernel-trace --stats` (counters are not collected) and adds one line with the
average time per call of the window kernels, the merge kernels among them.

    python tools/window_ext_cost.py [--conversations 100000] [--calls 10] [--configs 0,0x,1,4] [--full]
                                    [--profile] [--out profiles/window_ext/ext_cost.jsonl]
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

KERNELS = ("k_win_ext_count", "k_win_ext", "k_win_cands", "k_win_halo", "k_win_plan", "k_win_select", "k_win_alloc",
           "k_win_redact", "k_win_commit", "k_win_xmax", "k_win_jext", "k_scan_lb")


def pkg(mod):
    return importlib.import_module("context-based-pii_amd." + mod)


def candidates(lens, k, info_type, span_dtype):
    """k per row: start j * L // k, up to 8 bytes, inside the row (sorted by start; an empty row has none)"""
    n = len(lens)
    stride = max(1, k)
    spans = np.zeros((n, stride), dtype=span_dtype)
    if k:
        j = np.arange(k, dtype=np.int64)[None, :]
        L = lens.astype(np.int64)[:, None]
        s = j * L // k
        spans["start"] = s
        spans["end"] = np.minimum(L, s + 8)
        spans["info_type"] = info_type
        spans["likelihood"] = 4
        spans["utt"] = np.arange(n)[:, None]
    counts = np.where(lens > 0, k, 0).astype(np.uint32)
    return spans.reshape(-1), counts, stride


def run(a, out):
    import torch
    bench = importlib.import_module("bench")
    comp, E, synth = pkg("compiler"), pkg("engine"), pkg("synth")
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
    lens = (meta.offsets[1:] - meta.offsets[:-1]).astype(np.int64)
    step_bytes = [int(meta.offsets[(k + 1) * C] - meta.offsets[k * C]) for k in range(U)]
    blob = comp.compile_default().blob
    med = {}
    for name in a.configs.split(","):
        k = int(name.rstrip("x"))
        use_ext = name != "0"
        out_cap = (N + 1) * max(step_bytes) + 64 * N * C + 16 * N * C * k
        span_cap = (8 + k) * N * C
        d_out = torch.empty(out_cap, dtype=torch.uint8, device=dev)
        d_oo = torch.empty(C + 1, dtype=torch.int64, device=dev)
        d_sp = torch.empty(span_cap * 16, dtype=torch.uint8, device=dev)
        d_ctx = torch.empty(C, dtype=torch.int16, device=dev)
        eng = E.Engine(blob, device=0, n_conv_slots=C)
        eng.window_enable(N, 8192, full=a.full)
        person = eng.type_names.index("PERSON_NAME")
        spans, counts, stride = candidates(lens, k, person, E.SPAN_DTYPE)
        d_ext = torch.from_numpy(spans.view(np.uint8)).to(dev)
        d_ext_n = torch.from_numpy(counts.view(np.int32)).to(dev)
        torch.cuda.synchronize()
        ms, ob, ns = [], 0, 0
        for q in range(U):
            rows = (text.data_ptr(), offs.data_ptr() + 8 * q * C, C, int(meta.offsets[q * C]), step_bytes[q],
                    slot.data_ptr() + 4 * q * C, role.data_ptr() + q * C, ts.data_ptr() + 8 * q * C, d_out.data_ptr(),
                    out_cap, d_oo.data_ptr(), d_sp.data_ptr(), span_cap, d_ctx.data_ptr())
            if use_ext:
                eng.rescan_window_device_ext(*rows, d_ext.data_ptr() + 16 * q * C * stride, d_ext_n.data_ptr() + 4 * q * C,
                                             stride)
            else:
                eng.rescan_window_device_ex(*rows)
            ob, ns, flags = eng.sync()
            assert flags == 0, flags
            if q >= N:
                ms.append(eng.timings()[5])
        mode, scratch = eng.window_mode(), eng.scratch_bytes()
        eng.close()
        med[name] = statistics.median(ms)
        line = {"config": name, "candidates_per_row": k, "entry_point": "pii_rescan_window_device_" + ("ext" if use_ext else "ex"),
                "mode": mode, "rows_per_call": C, "new_bytes_per_call": step_bytes[-1], "window_bytes_out": int(ob),
                "window_findings": int(ns), "scratch_bytes": scratch, "call_ms": [round(x, 4) for x in ms],
                "call_ms_median": round(med[name], 4)}
        print(json.dumps(line), flush=True)
        out.append(line)
    if "0" in med and len(med) > 1:
        base = med["0"]
        line = {"baseline_call_ms": round(base, 4),
                **{f"{n}_minus_0_ms": round(v - base, 4) for n, v in med.items() if n != "0"},
                **{f"{n}_share_of_call": round((v - base) / base, 4) for n, v in med.items() if n != "0"}}
        print(json.dumps(line), flush=True)
        out.append(line)


def profile(a, out):
    """the same configurations in a child under rocprofv3: average ns per call of the window kernels"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--conversations", str(a.conversations), "--calls", str(a.calls), "--configs",
               a.profile_configs] + (["--full"] if a.full else [])
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
    line = {"rocprofv3_kernel_stats": True, "configs": a.profile_configs, "rows_per_call": a.conversations,
            "kernels": dict(sorted(per.items()))}
    print(json.dumps(line), flush=True)
    out.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conversations", type=int, default=100_000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--configs", default="0,0x,1,4")
    ap.add_argument("--full", action="store_true", help="force the full re-scan of the joined windows")
    ap.add_argument("--profile", action="store_true", help="only the rocprofv3 child run (kernel times)")
    ap.add_argument("--profile-configs", default="4")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    out = []
    (profile if a.profile else run)(a, out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for line in out:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
