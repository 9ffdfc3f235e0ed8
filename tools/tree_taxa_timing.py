"""qs_tree_taxon_agreement (per tree and taxon the quartet agreement with the reference) beside qs_tree_agreement of the same batch (the
kernel yardstick: it visits the same node pairs); run on a GPU box:
    python tools/tree_taxa_timing.py [out.json]          default profiles/r20_tree_taxa_timing.json
Two workloads, the ones of tools/tree_branch_timing.py: 512 taxa x 10 000 binary trees (the native generator) and 512 taxa x 1500 trees
with 20 % of the inner edges collapsed and 10 % of the taxa dropped (the numpy generator). Each is one child process of this script
under its own `timeout`, and the second starts only if the first ended well. Every figure is the best of 3 calls by HIP events around
the call on the context's stream, the three values kept; no table is allocated (neither call reads one). The only other route to the
same words, n + 1 calls of qs_tree_agreement on batches pruned and flattened again by the host, is not run: the JSON states
(n + 1) x the measured qs_tree_agreement beside the measured call. The child also holds the row sums against 4 x qs_tree_agreement;
correctness otherwise lives in tests/test_gpu_tree_taxa.py."""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = ("binary", "collapsed")


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
    m = batch.n_trees
    ctx = engine.Context(n, 16)
    hb = ctx.batch_upload(batch)
    s, keep = ctx._ref_struct(ref)
    rows = torch.empty(m * n * 4, dtype=torch.int64, device="cuda:0")
    agree = torch.empty(4 * m, dtype=torch.int64, device="cuda:0")
    taxa = lambda: ctx._chk(ctx.L.qs_tree_taxon_agreement(ctx.h, C.byref(s), hb, C.c_void_p(rows.data_ptr())))
    agreement = lambda: ctx._chk(ctx.L.qs_tree_agreement(ctx.h, C.byref(s), hb, C.c_void_p(agree.data_ptr())))
    taxa(); agreement(); ctx.sync()          # the first calls upload the reference
    taxa_ms, agree_ms = best_of_3(ctx, taxa), best_of_3(ctx, agreement)
    got = rows.cpu().numpy().reshape(m, n, 4)
    whole = agree.cpu().numpy().reshape(m, 4)
    ctx.batch_free(hb)
    del keep
    links = np.bincount(ref.parent[ref.parent >= 0], minlength=ref.n_nodes) + (ref.parent >= 0)
    ref_nodes = int((links >= 3).sum())
    pairs = int(np.diff(batch.node_off.astype(np.int64)).sum()) * ref_nodes
    best, yard = min(taxa_ms), min(agree_ms)
    print(json.dumps({
        "name": kind, "taxa": n, "trees": m, "plan": engine.tree_taxa_plan(n), "tree_taxa_ms": best, "tree_taxa_ms_calls": taxa_ms,
        "tree_agreement_ms": yard, "tree_agreement_ms_calls": agree_ms, "taxa_over_agreement": round(best / yard, 3),
        "node_pairs": pairs, "node_pairs_per_s": float(f"{pairs / (best * 1e-3):.4g}"),
        "agreement_route_ms_stated": round((n + 1) * yard, 1), "taxa_over_agreement_route": float(f"{best / ((n + 1) * yard):.3g}"),
        "row_sums_are_4x_agreement": bool((got.sum(1) == 4 * whole).all()),
        "sum_concordant": int(got[:, :, 0].sum()), "sum_discordant": int(got[:, :, 1].sum()), "sum_resolved_eval": int(got[:, :, 2].sum()),
        "sum_resolved_ref": int(got[:, :, 3].sum())}))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r20_tree_taxa_timing.json")
    results = []
    for kind in WORKLOADS:
        p = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", kind], capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(p.returncode)     # nothing more is started on the device
        results.append(json.loads(p.stdout.strip().splitlines()[-1]))
    line = json.dumps({"tool": "tree_taxa_timing", "results": results})
    print(line)
    with open(out_path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
