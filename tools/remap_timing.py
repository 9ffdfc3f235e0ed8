"""qs_table_remap + qs_score of a second reference tree against one recount, on configs[2]'s shape; run on a GPU box:
    python tools/remap_timing.py [taxa [trees]]          default 512 10000 (32-bit cells: the 34 GB table)
Counts once with reference A, re-indexes the table into a random reference B over the same taxa (best of 3 calls; the
identity permutation alongside = the same kernel with fully coalesced reads), scores B, recounts the trees once, checks
1e5 lookups of B's table against A's, and prints one JSON line. Effective bytes = one read + one write of the table."""
import json
import os
import sys
import time

import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quartetscores_amd import engine, flatten, native_ingest  # noqa: E402

HBM_TBPS = 8.0
n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
m = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
ref_a_nw = native_ingest.synth_trees(n, 1, 2000).decode().strip()
ref_b_nw = native_ingest.synth_trees(n, 1, 2002).decode().strip()
text = native_ingest.synth_trees(n, m, 2001)
ref_a, ref_b = flatten.flatten_reference(ref_a_nw), flatten.flatten_reference(ref_b_nw)
batch, _ = native_ingest.ingest_text(ref_a_nw, text, want_ranges=False)


def wall(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


src = engine.Context(n, 32)
src.table_alloc()
hb = src.batch_upload(batch, with_nodes=False)
src.count_batch(hb)
src.sync()
dst = engine.Context(n, 32)
dst.table_alloc()
dst.sync()
perm = flatten.taxon_permutation(ref_b, ref_a)


def remap(p):
    dst.table_remap(src, p)
    dst.sync()


remap_ms = [wall(lambda: remap(perm)) for _ in range(3)]
ident_ms = [wall(lambda: remap(np.arange(n))) for _ in range(3)]
remap(perm)
score_ms = [wall(lambda: dst.score(ref_b)) for _ in range(2)]
recount_ms = wall(lambda: (src.count_batch(hb, engine.QS_ALGO_AUTO | engine.QS_COUNT_OVERWRITE), src.sync()))
rng = np.random.default_rng(3)
q = np.stack([rng.choice(n, 4, replace=False) for _ in range(100000)])
lookups_match = bool((dst.lookup(q) == src.lookup(perm.astype(np.int64)[q])).all())
src.batch_free(hb)
bytes_moved = 2 * dst.table_bytes
best, best_ident = min(remap_ms), min(ident_ms)
tbps = bytes_moved / (best * 1e-3) / 1e12
print(json.dumps({
    "tool": "remap_timing", "taxa": n, "trees": m, "count_bits": 32, "table_bytes": dst.table_bytes,
    "remap_ms": round(best, 2), "remap_ms_calls": [round(x, 2) for x in remap_ms],
    "remap_identity_ms": round(best_ident, 2), "score_ms": round(min(score_ms), 2),
    "remap_plus_score_ms": round(best + min(score_ms), 2), "recount_ms": round(recount_ms, 2),
    "remap_plus_score_over_recount": round((best + min(score_ms)) / recount_ms, 3),
    "remap_effective_TBps": round(tbps, 3), "remap_hbm_roofline_frac": round(tbps / HBM_TBPS, 3),
    "remap_identity_effective_TBps": round(bytes_moved / (best_ident * 1e-3) / 1e12, 3),
    "lookups_match": lookups_match, "box_issue_probe_ns_per_inst": round(dst.issue_probe(), 4),
}))
