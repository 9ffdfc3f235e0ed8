"""qs_branch_frequencies (per node the trees that resolve a 4-set around its internode and the fixed-point sums of their normalised
frequencies: the inputs of --local-pp) beside qs_branch_resample with 16 replicates on the same rows (the yardstick: one read of the
same bytes, 16 multiply-adds per word where this kernel has three exact divisions per row) and qs_tree_branch_support of the same batch
(which writes the rows); run on a GPU box:
    python tools/local_pp_timing.py [out.json]          default profiles/r19_local_pp_timing.json
Two workloads, the ones of tools/tree_branch_timing.py: 512 taxa x 10 000 binary trees (the native generator) and 512 taxa x 1500 trees
with 20 % of the inner edges collapsed and 10 % of the taxa dropped (the numpy generator). Each is one child process of this script
under its own `timeout`, and the second starts only if the first ended well. Every figure is the best of 3 calls by HIP events around
the call on the context's stream, the three values kept. The sums of 8 nodes spread over the tree are held against big integers on the
host (tests/local_pp_model.py's rule); correctness at large lives in tests/test_gpu_local_pp.py."""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = ("binary", "collapsed")
REPS = 16
ONE = 1 << 40


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
    sums = torch.zeros(REPS * N * 4, dtype=torch.int64, device="cuda:0")
    freq = torch.zeros(N * 4, dtype=torch.int64, device="cuda:0")
    w = np.random.default_rng(1).multinomial(m, np.full(m, 1.0 / m), size=REPS).astype(np.uint32)
    branch = lambda: ctx._chk(ctx.L.qs_tree_branch_support(ctx.h, C.byref(s), hb, C.c_void_p(rows.data_ptr())))
    resample = lambda: ctx._chk(ctx.L.qs_branch_resample(ctx.h, C.c_void_p(rows.data_ptr()), m, N, w.ctypes.data_as(C.c_void_p), REPS,
                                                         C.c_void_p(sums.data_ptr())))
    frequencies = lambda: ctx._chk(ctx.L.qs_branch_frequencies(ctx.h, C.c_void_p(rows.data_ptr()), m, N, C.c_void_p(freq.data_ptr())))
    branch(); resample(); frequencies(); ctx.sync()          # the first calls upload the reference and load the code
    branch_ms, resample_ms, freq_ms = best_of_3(ctx, branch), best_of_3(ctx, resample), best_of_3(ctx, frequencies)
    calls = 1 + 3                                             # every call added the batch once more
    got = freq.cpu().numpy().reshape(N, 4)
    host = rows.cpu().numpy().reshape(m, N, 4)
    ctx.batch_free(hb)
    del keep
    resolved = np.nonzero(got[:, 0])[0]
    picked = resolved[np.linspace(0, len(resolved) - 1, 8).astype(int)] if len(resolved) else resolved
    for v in picked.tolist():
        want = [0, 0, 0, 0]
        for _, q1, q2, q3 in host[:, v].tolist():
            if q1 + q2 + q3 > 0:
                want[0] += 1
                for i, q in enumerate((q1, q2, q3)):
                    want[1 + i] += q * ONE // (q1 + q2 + q3)
        if got[v].tolist() != [calls * x for x in want]:
            sys.exit(f"node {v}: {got[v].tolist()} is not {calls} x {want}")
    best, bytes_read = min(freq_ms), m * N * 32
    print(json.dumps({
        "name": kind, "taxa": n, "trees": m, "nodes": N, "resolved_nodes": int(len(resolved)), "row_bytes": bytes_read,
        "frequencies_ms": best, "frequencies_ms_calls": freq_ms, "frequencies_gb_per_s": float(f"{bytes_read / (best * 1e-3) / 1e9:.4g}"),
        "resample_reps": REPS, "resample_ms": min(resample_ms), "resample_ms_calls": resample_ms,
        "frequencies_over_resample": round(best / min(resample_ms), 3),
        "tree_branch_ms": min(branch_ms), "tree_branch_ms_calls": branch_ms, "frequencies_over_tree_branch": float(f"{best / min(branch_ms):.3g}"),
        "checked_nodes": picked.tolist(), "sum_en": int(got[:, 0].sum()) // calls}))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r19_local_pp_timing.json")
    results = []
    for kind in WORKLOADS:
        p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", kind], capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(p.returncode)     # nothing more is started on the device
        results.append(json.loads(p.stdout.strip().splitlines()[-1]))
    line = json.dumps({"tool": "local_pp_timing", "results": results})
    print(line)
    with open(out_path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
