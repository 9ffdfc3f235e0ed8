"""qs_group_support beside the per-taxon pass and the old route for one hypothesis, on configs[2]'s shape; run on a GPU box:
    python tools/group_support_timing.py [taxa [trees [out.json]]]    default 512 10000 profiles/r12_group_support_timing.json
Counts once (32-bit cells: the 34 GB table), then times -- each best of 3 calls by the host clock around call + sync, the download of
6 words per hypothesis included -- one quad hypothesis from the four subtrees beside the most central edge of the benchmark's
reference tree, one split hypothesis of the first against the second half of the taxa, and HG and 8 HG random hypotheses of either
kind in which every taxon takes part (HG = 8 hypotheses share one read of the table). The two yardsticks on the same table: one
qs_taxon_support pass (one read of the table in the same load shape), and the old route for ONE hypothesis: qs_table_remap into
the lookup ids of a candidate tree that has the branch + qs_score of that tree. Checks the quartets word of every hypothesis against
qs_group_check, and the central edge's log_score(q1, q2, q3) against qs_score's qp-ic of that edge. Prints one JSON line and
writes it to out.json."""
import json
import os
import sys
import time

import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quartetscores_amd import engine, flatten, native_ingest  # noqa: E402

HG = 8
args = sys.argv[1:]
n = int(args[0]) if len(args) > 0 else 512
m = int(args[1]) if len(args) > 1 else 10000
out_path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "r12_group_support_timing.json")
ref_nw = native_ingest.synth_trees(n, 1, 2000).decode().strip()
text = native_ingest.synth_trees(n, m, 2001)
ref = flatten.flatten_reference(ref_nw)
batch, _ = native_ingest.ingest_text(ref_nw, text, want_ranges=False)


def wall(f):
    t = time.perf_counter()
    r = f()
    return (time.perf_counter() - t) * 1e3, r


def best_of(f, calls=3):
    f()                                  # warm: plans, code objects
    ms = [wall(f) for _ in range(calls)]
    assert all((r == ms[0][1]).all() for _, r in ms)
    return [t for t, _ in ms], ms[0][1]


def central_edge(ref):
    """the inner edge of the (binary, unrooted) reference whose smaller side is largest -> (child node, label row S1 S2 | S3 S4)"""
    parent, _, lo, hi, _, root = engine._tree_arrays(ref)
    N = len(parent)
    kids = [[] for _ in range(N)]
    for v in range(N):
        if parent[v] >= 0:
            kids[parent[v]].append(v)
    inner = [v for v in range(N) if v != root and len(kids[v]) == 2]
    v = max(inner, key=lambda x: min(hi[x] - lo[x], n - (hi[x] - lo[x])))
    p = int(parent[v])
    row = np.zeros(n, dtype=np.uint8)
    sides = [c for c in kids[p] if c != v]
    if p != root:
        row[:] = 4                       # everything outside the parent's subtree
        row[lo[sides[0]]:hi[sides[0]]] = 3
    else:
        row[lo[sides[0]]:hi[sides[0]]], row[lo[sides[1]]:hi[sides[1]]] = 3, 4
    x, y = sorted(kids[v], key=lambda c: lo[c])
    row[lo[x]:hi[x]], row[lo[y]:hi[y]] = 1, 2
    return v, row


ctx = engine.Context(n, 32)
ctx.table_alloc()
hb = ctx.batch_upload(batch, with_nodes=False)
ctx.count_batch(hb)
ctx.sync()
ctx.batch_free(hb)

rng = np.random.default_rng(2012)
edge, quad_row = central_edge(ref)
split_row = np.where(np.arange(n) < n // 2, 1, 2).astype(np.uint8)
cases = {
    "quad_central_edge": quad_row[None, :], "split_halves": split_row[None, :],
    "quad_x_HG": rng.integers(1, 5, size=(HG, n)).astype(np.uint8), "split_x_HG": rng.integers(1, 3, size=(HG, n)).astype(np.uint8),
    "quad_x_8HG": rng.integers(1, 5, size=(8 * HG, n)).astype(np.uint8), "split_x_8HG": rng.integers(1, 3, size=(8 * HG, n)).astype(np.uint8),
}
out = {"tool": "group_support_timing", "taxa": n, "trees": m, "count_bits": 32, "table_bytes": ctx.table_bytes, "HG": HG, "cases": {}}
quartets_ok = True
for name, labels in cases.items():
    ms, words = best_of(lambda: ctx.group_support(labels))
    quartets_ok = quartets_ok and bool((words[:, 0].astype(np.uint64) == engine.group_check(n, labels)[1]).all())
    passes = (len(labels) + HG - 1) // HG
    out["cases"][name] = {"hypotheses": len(labels), "passes": passes, "ms": round(min(ms), 2), "ms_calls": [round(x, 2) for x in ms],
                          "ms_per_hypothesis": round(min(ms) / len(labels), 3), "ms_per_pass": round(min(ms) / passes, 2),
                          "counted_4sets_mean": float(np.mean(words[:, 0].astype(np.float64))),
                          "effective_TBps_per_pass": round(ctx.table_bytes / (min(ms) / passes * 1e-3) / 1e12, 3)}
central = ctx.group_support(quad_row[None, :])[0]

taxon_ms, _ = best_of(lambda: ctx.taxon_support(ref))
qpic = ctx.score(ref, engine.QS_SCORE_QP_EXACT64)[1]
# S3 / S4 are not put in the order of qs_score's frame here: the two orders of (q2, q3) may differ in the last bits
mine = [engine.log_score(int(central[1]), int(central[a]), int(central[b])) for a, b in ((2, 3), (3, 2))]
edge_matches = bool(any(np.float64(x).view(np.int64) == np.float64(qpic[edge]).view(np.int64) for x in mine))

# the old route for one hypothesis: a candidate tree that has the branch, the table re-indexed into its ids, its scores
cand_nw = native_ingest.synth_trees(n, 1, 2002).decode().strip()
cand = flatten.flatten_reference(cand_nw)
perm = flatten.taxon_permutation(cand, ref)
dst = engine.Context(n, 32)
dst.table_alloc()
dst.sync()
dst.table_remap(ctx, perm); dst.sync(); dst.score(cand)     # warm
remap_ms = [wall(lambda: (dst.table_remap(ctx, perm), dst.sync()))[0] for _ in range(3)]
score_ms = [wall(lambda: dst.score(cand))[0] for _ in range(3)]
dst.close()

one_pass = out["cases"]["quad_x_HG"]["ms"]
old = min(remap_ms) + min(score_ms)
out.update({
    "taxon_support_ms": round(min(taxon_ms), 2), "taxon_support_ms_calls": [round(x, 2) for x in taxon_ms],
    "old_route_remap_ms": round(min(remap_ms), 2), "old_route_score_ms": round(min(score_ms), 2), "old_route_ms_per_hypothesis": round(old, 2),
    "pass_of_HG_quads_over_taxon_support": round(one_pass / min(taxon_ms), 3),
    "pass_of_HG_splits_over_taxon_support": round(out["cases"]["split_x_HG"]["ms"] / min(taxon_ms), 3),
    "old_route_over_per_hypothesis_at_8HG": round(old / out["cases"]["quad_x_8HG"]["ms_per_hypothesis"], 1),
    "old_route_over_one_hypothesis_alone": round(old / out["cases"]["quad_central_edge"]["ms"], 2),
    "quartets_match_group_check": quartets_ok, "central_edge_node": int(edge), "central_edge_words": [int(x) for x in central],
    "central_edge_qpic_matches_qs_score": edge_matches,
    "box_issue_probe_ns_per_inst": round(ctx.issue_probe(), 4),
})
ctx.close()
line = json.dumps(out)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(line + "\n")
