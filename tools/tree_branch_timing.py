"""qs_tree_branch_support (per tree the quartet support of every reference internode) beside qs_tree_agreement of the same batch (the
kernel yardstick: it visits the same node pairs) and qs_branch_resample at B = 100; run on a GPU box:
    python tools/tree_branch_timing.py [out.json]          default profiles/r18_tree_branch_timing.json
Two workloads, the ones of tools/agreement_timing.py: 512 taxa x 10 000 binary trees (the native generator) and 512 taxa x 1500 trees
with 20 % of the inner edges collapsed and 10 % of the taxa dropped (the numpy generator). Each is one child process of this script
under its own `timeout`, and the second starts only if the first ended well. Every figure is the best of 3 calls by HIP events around
the call on the context's stream, the three values kept; no table is allocated (neither call reads one). The feature yardstick, one
count of a tree alone plus a totals pass per tree (about 10 ms of score pass each), is not run: the JSON states
m x 10 ms beside the measured call. Correctness lives in tests/test_gpu_tree_branch.py."""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = ("binary", "collapsed")
REPS = 100


def best_of_3(ctx, call):
    import torch
    ms = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        call()
        b.record()
        ctx.sync()
        torch.cuda.synchronize()
        ms.append(round(a.elapsed_time(b), 3))
    return ms


def child(kind):
    import numpy as np
    import torch
    from quartetscores_amd import engine, flatten, native_ingest, synth
    n = 512
    if kind == "binary":
        ref_nw = native_ingest.synth_trees(n, 1, 2000).decode().strip()
        batch, _ = native_ingest.ingest_text(ref_nw, native_ingest.synth_trees(n, 10000, 2001), want_ranges=True)
    else:
        rng = np.random.default_rng(7)
        ref_nw = synth.random_tree(n, rng)
        trees = [synth.random_tree(n, rng, collapse=0.2, dropout=0.1) for _ in range(1500)]
        batch = flatten.flatten_eval_trees(trees, flatten.flatten_reference(ref_nw).name_to_id)
    ref = flatten.flatten_reference(ref_nw)
    m, N = batch.n_trees, ref.n_nodes
    ctx = engine.Context(n, 16)
    hb = ctx.batch_upload(batch)
    s, keep = ctx._ref_struct(ref)
    rows = torch.empty(m * N * 4, dtype=torch.int64, device="cuda:0")
    agree = torch.empty(4 * m, dtype=torch.int64, device="cuda:0")
    sums = torch.zeros(REPS * N * 4, dtype=torch.int64, device="cuda:0")
    w = np.random.default_rng(1).multinomial(m, np.full(m, 1.0 / m), size=REPS).astype(np.uint32)
    branch = lambda: ctx._chk(ctx.L.qs_tree_branch_support(ctx.h, C.byref(s), hb, C.c_void_p(rows.data_ptr())))
    agreement = lambda: ctx._chk(ctx.L.qs_tree_agreement(ctx.h, C.byref(s), hb, C.c_void_p(agree.data_ptr())))
    resample = lambda: ctx._chk(ctx.L.qs_branch_resample(ctx.h, C.c_void_p(rows.data_ptr()), m, N, w.ctypes.data_as(C.c_void_p), REPS,
                                                         C.c_void_p(sums.data_ptr())))
    branch(); agreement(); ctx.sync()          # the first calls upload the reference
    branch_ms, agree_ms = best_of_3(ctx, branch), best_of_3(ctx, agreement)
    resample_ms = best_of_3(ctx, resample)
    got = rows.cpu().numpy().reshape(m, N, 4)
    ctx.batch_free(hb)
    del keep
    internodes = int((got[:, :, 0].max(0) > 0).sum())
    pairs = int(np.diff(batch.node_off.astype(np.int64)).sum()) * internodes
    best = min(branch_ms)
    print(json.dumps({
        "name": kind, "taxa": n, "trees": m, "internode_entries": internodes, "tree_branch_ms": best, "tree_branch_ms_calls": branch_ms,
        "tree_agreement_ms": min(agree_ms), "tree_agreement_ms_calls": agree_ms, "branch_over_agreement": round(best / min(agree_ms), 3),
        "node_pairs": pairs, "node_pairs_per_s": float(f"{pairs / (best * 1e-3):.4g}"),
        "resample_reps": REPS, "resample_ms": min(resample_ms), "resample_ms_calls": resample_ms,
        "recount_route_ms_stated": m * 10.0, "branch_over_recount_route": float(f"{best / (m * 10.0):.3g}"),
        "sum_present": int(got[:, :, 0].sum()), "sum_q1": int(got[:, :, 1].sum()), "sum_q2": int(got[:, :, 2].sum()), "sum_q3": int(got[:, :, 3].sum())}))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r18_tree_branch_timing.json")
    results = []
    for kind in WORKLOADS:
        p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", kind], capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(p.returncode)     # nothing more is started on the device
        results.append(json.loads(p.stdout.strip().splitlines()[-1]))
    line = json.dumps({"tool": "tree_branch_timing", "results": results})
    print(line)
    with open(out_path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
