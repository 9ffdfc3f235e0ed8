"""qs_tree_pair_agreement (quartet agreement of the evaluation trees with each other) against qs_tree_agreement as the yardstick;
run on a GPU box:
    python tools/tree_pairs_timing.py [out.json]
Three workloads in ONE process, warmed up once each and then alternating, best of 3 by the host clock around call + sync:
  pairs_binary   512 taxa x 1000 binary trees (the native generator), upper triangle: 499 500 pairs
  pairs_mixed    512 taxa x 300 trees with 20 % of the inner edges collapsed and 10 % of the taxa dropped, upper triangle
  yardstick      qs_tree_agreement of 512 taxa x 10 000 binary trees against the reference tree (profiles/r07_agreement_timing.json)
For each the node pairs it evaluates (inner nodes of the one tree x inner nodes of the other, summed over the pairs of trees) and node
pairs per second; `ratio` = a pair workload's rate over the yardstick's of the same run. Prints one JSON line (correctness lives in
tests/test_gpu_tree_pairs.py; the binary workload's words are checked against C(512,4) here because it costs nothing)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quartetscores_amd import _lib, engine, flatten, native_ingest, synth  # noqa: E402


def upper_node_pairs(batch):
    inner = np.diff(batch.node_off.astype(np.int64))
    return int((int(inner.sum()) ** 2 - int((inner * inner).sum())) // 2)


def main():
    n = 512
    ref_nw = native_ingest.synth_trees(n, 1, 2000).decode().strip()
    ref = flatten.flatten_reference(ref_nw)
    ctx = engine.Context(n)
    big, _ = native_ingest.ingest_text(ref_nw, native_ingest.synth_trees(n, 10000, 2001), want_ranges=True)
    binary, _ = native_ingest.ingest_text(ref_nw, native_ingest.synth_trees(n, 1000, 2002), want_ranges=True)
    rng = np.random.default_rng(7)
    mixed = flatten.flatten_eval_trees([synth.random_tree(n, rng, collapse=0.2, dropout=0.1) for _ in range(300)], ref.name_to_id)
    hb_big, hb_bin, hb_mix = ctx.batch_upload(big), ctx.batch_upload(binary), ctx.batch_upload(mixed)
    buf_agree = torch.empty(4 * big.n_trees, dtype=torch.int64, device="cuda:0")
    buf_pairs = torch.empty(5 * binary.n_trees ** 2, dtype=torch.int64, device="cuda:0")
    s, keep = ctx._ref_struct(ref)
    ref_inner = sum(1 for u in range(ref.n_nodes) if (ref.parent == u).sum() + (ref.parent[u] >= 0) >= 3)

    def pairs(hb, m):
        ctx._chk(ctx.L.qs_tree_pair_agreement(ctx.h, hb, 0, m, hb, 0, m, _lib.QS_PAIRS_UPPER, C.c_void_p(buf_pairs.data_ptr())))

    work = {
        "pairs_binary": (lambda: pairs(hb_bin, binary.n_trees), upper_node_pairs(binary), binary.n_trees),
        "pairs_mixed": (lambda: pairs(hb_mix, mixed.n_trees), upper_node_pairs(mixed), mixed.n_trees),
        "yardstick": (lambda: ctx._chk(ctx.L.qs_tree_agreement(ctx.h, C.byref(s), hb_big, C.c_void_p(buf_agree.data_ptr()))),
                      int(np.diff(big.node_off.astype(np.int64)).sum()) * ref_inner, big.n_trees),
    }
    order = ["pairs_binary", "yardstick", "pairs_mixed"]
    ms = {k: [] for k in work}
    checks = {}
    for rep in range(4):   # rep 0 warms up
        for name in order:
            ctx.sync()
            t = time.perf_counter()
            work[name][0]()
            ctx.sync()
            dt = (time.perf_counter() - t) * 1e3
            if rep:
                ms[name].append(dt)
            elif name == "pairs_binary":
                m = binary.n_trees
                w = buf_pairs[: 5 * m * m].cpu().numpy().view(np.uint64).reshape(m, m, 5)
                up = np.triu(np.ones((m, m), dtype=bool), 1)
                full = n * (n - 1) * (n - 2) * (n - 3) // 24
                checks["binary_words_ok"] = bool(((w[up][:, 0] + w[up][:, 1]) == full).all() and (w[up][:, 2:4] == full).all()
                                                 and (w[up][:, 4] == n).all() and (w[~up] == 0).all())
                checks["binary_mean_distance"] = float(f"{(w[up][:, 1].astype(np.float64) / full).mean():.6f}")
    out = []
    for name, (_, node_pairs, trees) in work.items():
        best = min(ms[name])
        out.append({"name": name, "taxa": n, "trees": trees, "ms": round(best, 3), "ms_calls": [round(x, 3) for x in ms[name]],
                    "node_pairs": node_pairs, "node_pairs_per_s": float(f"{node_pairs / (best * 1e-3):.4g}")})
    yard = out[-1]["node_pairs_per_s"]
    for r in out[:-1]:
        r["ratio_to_yardstick"] = round(r["node_pairs_per_s"] / yard, 4)
    del keep
    line = json.dumps({"tool": "tree_pairs_timing", "results": out, **checks})
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
