#!/usr/bin/env python3
"""What re-identification costs ("Re-identification: what the call costs").

The 9731-row test corpus (synth.build_bank(600, 600, seed=7), make_corpus(263, 37, seed=3)) tiled to about a
million rows, each tile with conversation slots of its own, in device buffers, under one catch-all
crypto_replace_ffx_fpe_config (ALPHA_NUMERIC, a 16-byte key: the tests' FC).  Three calls are timed with events
on one stream, after a warm-up round, interleaved round by round so that drift hits all three alike:

    scan      pii_scan_redact_device over the rows (what de-identifying them cost)
    reid_out  pii_reidentify_device over its output and spans, into another buffer (one device-to-device copy first)
    reid_in   pii_reidentify_device in place

Each round's scan writes the rows and spans the two re-identify calls of that round read.  One JSON line per call
(median, min, max of --rounds rounds, milliseconds) and a summary line with the copy's bytes are appended to --out.

    python tools/reid_cost.py [--tiles 103] [--rounds 9] [--out profiles/reidentify/reid_cost.jsonl]
"""
import argparse
import base64
import importlib
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pkg(mod):
    return importlib.import_module("context-based-pii_amd." + mod)


FPE_C = [{"primitive_transformation": {"crypto_replace_ffx_fpe_config": {"crypto_key": {"unwrapped": {
    "key": base64.b64encode(bytes(range(16))).decode()}}, "common_alphabet": "ALPHA_NUMERIC"}}}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=103)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reidentify", "reid_cost.jsonl"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("reid_cost.py measures on the GPU; no device found")
    comp, E, synth = pkg("compiler"), pkg("engine"), pkg("synth")
    corp = synth.make_corpus(263, 37, synth.build_bank(600, 600, seed=7), seed=3)
    n1, b1 = corp.n, int(corp.offsets[-1])
    n_conv = int(corp.conv_slot.max()) + 1
    n, total = n1 * a.tiles, b1 * a.tiles
    data = np.tile(corp.data[:b1], a.tiles)
    lens = np.tile(np.diff(corp.offsets.astype(np.int64)), a.tiles)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    slot = (np.tile(corp.conv_slot.astype(np.int64), a.tiles) + np.repeat(np.arange(a.tiles), n1) * n_conv).astype(np.uint32)
    role, ts = np.tile(corp.role, a.tiles), np.tile(corp.ts_us, a.tiles)
    with open(os.path.join(comp.RULES_DIR, "dlp_config.json")) as f:
        cfg = json.load(f)
    cfg["deidentify_config"] = {"info_type_transformations": {"transformations": FPE_C}}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "fc.json")
        with open(path, "w") as f:
            json.dump(cfg, f)
        blob = comp.compile_default(path).blob
    dev = torch.device("cuda:0")
    d_text = torch.from_numpy(np.concatenate([data, np.zeros(64, np.uint8)])).to(dev)
    d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
    d_slot = torch.from_numpy(slot.view(np.int32)).to(dev)
    d_role = torch.from_numpy(np.ascontiguousarray(role, dtype=np.uint8)).to(dev)
    d_ts = torch.from_numpy(np.ascontiguousarray(ts, dtype=np.int64)).to(dev)
    out_cap, span_cap = total + 64, n
    d_out = torch.empty(out_cap + 32, dtype=torch.uint8, device=dev)
    d_re = torch.empty(out_cap + 32, dtype=torch.uint8, device=dev)
    d_oo = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_sp = torch.empty(span_cap * 16, dtype=torch.uint8, device=dev)
    d_ctx = torch.empty(n, dtype=torch.int16, device=dev)
    d_status = torch.zeros(2, dtype=torch.int32, device=dev)
    eng = E.Engine(blob, device=0, n_conv_slots=n_conv * a.tiles)
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    ms = {"scan": [], "reid_out": [], "reid_in": []}
    ob = ns = 0

    def timed(name, call, keep):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        if keep:
            ms[name].append(e0.elapsed_time(e1))

    def scan():
        eng.scan_redact_device_ex(d_text.data_ptr(), d_offs.data_ptr(), n, 0, total, d_slot.data_ptr(), d_role.data_ptr(),
                                  d_ts.data_ptr(), d_out.data_ptr(), out_cap, d_oo.data_ptr(), d_sp.data_ptr(), span_cap,
                                  d_ctx.data_ptr(), stream=st)

    for rnd in range(1 + a.rounds):                   # round 0 warms every call up
        timed("scan", scan, rnd > 0)
        ob, ns, flags = eng.sync()
        assert flags == 0 and ob == total, (flags, ob, total)      # FC keeps every row's length
        timed("reid_out", lambda: eng.reidentify_device(d_out.data_ptr(), d_oo.data_ptr(), n, 0, ob, d_sp.data_ptr(), ns,
                                                        d_re.data_ptr(), out_cap, d_status.data_ptr(), stream=st), rnd > 0)
        timed("reid_in", lambda: eng.reidentify_device(d_out.data_ptr(), d_oo.data_ptr(), n, 0, ob, d_sp.data_ptr(), ns,
                                                       d_out.data_ptr(), out_cap, d_status.data_ptr() + 4, stream=st),
              rnd > 0)
        assert d_status.cpu().tolist() == [0, 0]
    # FC re-identifies to the input: the timed calls computed what they are meant to
    same_out = bool(torch.equal(d_re[:total], d_text[:total]))
    same_in = bool(torch.equal(d_out[:total], d_text[:total]))
    eng.close()
    assert same_out and same_in
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    med = {k: statistics.median(v) for k, v in ms.items()}
    with open(a.out, "a") as f:
        for k, v in ms.items():
            line = json.dumps({"call": k, "rows": n, "bytes": total, "spans": int(ns), "rounds": a.rounds,
                               "ms_median": round(med[k], 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                               "ms": [round(x, 4) for x in v]})
            print(line, flush=True)
            f.write(line + "\n")
        line = json.dumps({"summary": "out of place minus in place", "ms": round(med["reid_out"] - med["reid_in"], 4),
                           "copy_bytes_read_plus_written": 2 * total,
                           "copy_gbps_if_all_of_it": round(2 * total / max(med["reid_out"] - med["reid_in"], 1e-6) / 1e6, 1),
                           "reid_in_ns_per_span": round(med["reid_in"] * 1e6 / max(int(ns), 1), 2),
                           "restored_equals_input": same_out and same_in})
        print(line, flush=True)
        f.write(line + "\n")


if __name__ == "__main__":
    main()
