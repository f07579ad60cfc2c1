#!/usr/bin/env python3
"""What crypto_replace_ffx_fpe_config costs in the redaction path ("crypto_replace_ffx_fpe_config").

The batch of tools/xf_hash_cost.py (conversation-major rows from the synth bank, in device buffers), run
through four engines: the shipped config ("[TYPE]" tokens), one catch-all character mask, one catch-all
crypto_hash_config and one catch-all crypto_replace_ffx_fpe_config (ALPHA_NUMERIC, a 16-byte key).  Per engine:
kernel_timings()["k_redact"] (k_redact plus the k_mask / k_hash / k_fpe post-pass), median of --calls calls
after one warm-up call.  k_fpe's own time is the FPE median minus the shipped one.  The AES blocks it ran are
counted from the findings' numerals: one for P, and per round one for Q (two where b(v) = 16) and one more
where d = 20 (b(v) > 12); a finding that falls back runs none.  One JSON line per engine and a summary line.

    python tools/xf_fpe_cost.py [--conversations 30000] [--rows-per-conversation 20] [--calls 5]
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


MASK_B = [{"primitive_transformation": {"character_mask_config": {"masking_character": "*", "characters_to_ignore": [
    {"common_characters_to_ignore": "PUNCTUATION"}, {"common_characters_to_ignore": "WHITESPACE"}]}}}]
HASH_C = [{"primitive_transformation": {"crypto_hash_config": {"crypto_key": {"unwrapped": {
    "key": base64.b64encode(bytes(range(32))).decode()}}}}}]
ALPHABET = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"
FPE_C = [{"primitive_transformation": {"crypto_replace_ffx_fpe_config": {"crypto_key": {"unwrapped": {
    "key": base64.b64encode(bytes(range(16))).decode()}}, "common_alphabet": "ALPHA_NUMERIC"}}}]
BLOCKS = [("shipped", None), ("mask_catch_all", MASK_B), ("hash_catch_all", HASH_C), ("fpe_catch_all", FPE_C)]


def aes_blocks(comp, numerals):
    """AES blocks ff1_apply runs for findings of these numeral counts (ALPHABET), and how many fall back"""
    radix = len(ALPHABET)
    nmin, nmax = comp.fpe_limits(radix)
    blocks = fell = 0
    for n, count in zip(*np.unique(numerals, return_counts=True)):
        n = int(n)
        if not nmin <= n <= nmax:
            fell += int(count)
            continue
        b = ((radix ** (n - n // 2) - 1).bit_length() + 7) // 8
        blocks += int(count) * (1 + 10 * ((2 if b == 16 else 1) + (1 if b > 12 else 0)))
    return blocks, fell


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conversations", type=int, default=30000)
    ap.add_argument("--rows-per-conversation", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    import torch
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
    with open(os.path.join(comp.RULES_DIR, "dlp_config.json")) as f:
        shipped = json.load(f)
    med, blocks, fell = {}, 0, 0
    is_numeral = np.zeros(256, dtype=np.int64)
    is_numeral[np.frombuffer(ALPHABET.encode(), dtype=np.uint8)] = 1
    numeral_sum = np.concatenate([[0], np.cumsum(is_numeral[corp.data])])
    for name, block in BLOCKS:
        cfg = dict(shipped)
        if block is not None:
            cfg["deidentify_config"] = {"info_type_transformations": {"transformations": block}}
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, name + ".json")
            with open(path, "w") as f:
                json.dump(cfg, f)
            blob = comp.compile_default(path).blob
        ms = []
        eng = E.Engine(blob, device=0, n_conv_slots=a.conversations)
        for _ in range(1 + a.calls):
            eng.scan_redact_device(d_text.data_ptr(), d_offs.data_ptr(), n, d_slot.data_ptr(), d_role.data_ptr(),
                                   d_ts.data_ptr(), d_out.data_ptr(), out_cap, d_oo.data_ptr(), d_sp.data_ptr(),
                                   span_cap, d_ctx.data_ptr())
            ob, ns, flags = eng.sync()
            assert flags == 0, flags
            ms.append(eng.kernel_timings()["k_redact"])
        lane_bytes = eng.stats()["lane_bytes"]
        eng.close()
        spans = np.frombuffer(d_sp[:ns * 16].cpu().numpy().tobytes(), dtype=E.SPAN_DTYPE)
        lens = spans["end"].astype(np.int64) - spans["start"].astype(np.int64)
        at = corp.offsets[spans["utt"].astype(np.int64)].astype(np.int64)
        numerals = numeral_sum[at + spans["end"].astype(np.int64)] - numeral_sum[at + spans["start"].astype(np.int64)]
        blocks, fell = aes_blocks(comp, numerals)
        med[name] = statistics.median(ms[1:])
        print(json.dumps({"config": name, "rows": n, "bytes_in": total, "bytes_out": ob, "findings": int(ns),
                          "finding_bytes": int(lens.sum()), "lane_bytes": lane_bytes,
                          "k_redact_ms": [round(x, 4) for x in ms[1:]], "k_redact_ms_median": round(med[name], 4)}),
              flush=True)
    k_fpe_ms = med["fpe_catch_all"] - med["shipped"]
    print(json.dumps({"k_fpe_ms": round(k_fpe_ms, 4), "k_hash_ms": round(med["hash_catch_all"] - med["shipped"], 4),
                      "k_mask_ms": round(med["mask_catch_all"] - med["shipped"], 4), "findings": int(ns),
                      "fell_back": fell, "aes_blocks": blocks, "aes_blocks_per_finding": round(blocks / max(int(ns), 1), 2),
                      "aes_blocks_per_s": round(blocks / (k_fpe_ms * 1e-3)) if k_fpe_ms > 0 else None}))


if __name__ == "__main__":
    main()
