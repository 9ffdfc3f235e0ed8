"""qs_tree_agreement (per-tree quartet agreement with the reference tree) against one count pass; run on a GPU box:
    python tools/agreement_timing.py [out.json]
Two workloads: BASELINE configs[2] (512 taxa x 10 000 binary trees, the native generator) and 512 taxa x 1500 trees with
20 % of the inner edges collapsed and 10 % of the taxa dropped (the numpy generator). For each: the agreement call's device
time (best of 3, HIP events around the launch), the node pairs it evaluates, node pairs per second, and one count pass of the
same batch (QS_COUNT_OVERWRITE) for scale. Prints one JSON line (correctness lives in tests/test_gpu_tree_agreement.py)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quartetscores_amd import engine, flatten, native_ingest, synth  # noqa: E402


def measure(name, ref_nw, batch, n, count_bits):
    ref = flatten.flatten_reference(ref_nw)
    ctx = engine.Context(n, count_bits)
    ctx.table_alloc()
    hb = ctx.batch_upload(batch)
    m = batch.n_trees
    buf = torch.empty(4 * m, dtype=torch.int64, device="cuda:0")
    s, keep = ctx._ref_struct(ref)
    ctx._chk(ctx.L.qs_tree_agreement(ctx.h, C.byref(s), hb, C.c_void_p(buf.data_ptr())))   # first call uploads the reference
    ctx.sync()
    ms = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        ctx._chk(ctx.L.qs_tree_agreement(ctx.h, C.byref(s), hb, C.c_void_p(buf.data_ptr())))
        b.record()
        ctx.sync()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    got = buf.cpu().numpy().view(np.uint64).reshape(m, 4)
    t = time.perf_counter()
    ctx.count_batch(hb, engine.QS_ALGO_AUTO | engine.QS_COUNT_OVERWRITE)
    ctx.sync()
    count_ms = (time.perf_counter() - t) * 1e3
    ctx.batch_free(hb)
    ref_inner = sum(1 for u in range(ref.n_nodes) if (ref.parent == u).sum() + (ref.parent[u] >= 0) >= 3)
    eval_inner = np.diff(batch.node_off.astype(np.int64))
    pairs = int(eval_inner.sum()) * ref_inner
    best = min(ms)
    return {"name": name, "taxa": n, "trees": m, "agreement_ms": round(best, 3), "agreement_ms_calls": [round(x, 3) for x in ms],
            "node_pairs": pairs, "node_pairs_per_s": float(f"{pairs / (best * 1e-3):.4g}"), "count_pass_ms": round(count_ms, 2),
            "agreement_over_count": round(best / count_ms, 4), "sum_concordant": int(got[:, 0].sum()), "sum_discordant": int(got[:, 1].sum())}


def main():
    n = 512
    out = []
    ref_nw = native_ingest.synth_trees(n, 1, 2000).decode().strip()
    text = native_ingest.synth_trees(n, 10000, 2001)
    batch, _ = native_ingest.ingest_text(ref_nw, text, want_ranges=True)
    out.append(measure("configs[2] binary", ref_nw, batch, n, 32))
    rng = np.random.default_rng(7)
    ref2 = synth.random_tree(n, rng)
    trees = [synth.random_tree(n, rng, collapse=0.2, dropout=0.1) for _ in range(1500)]
    ref2_flat = flatten.flatten_reference(ref2)
    out.append(measure("collapse0.2+dropout0.1", ref2, flatten.flatten_eval_trees(trees, ref2_flat.name_to_id), n, 16))
    line = json.dumps({"tool": "agreement_timing", "results": out})
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
