"""qs_table_restrict + qs_score of the reference tree without some taxa against one recount of the pruned trees, on
configs[2]'s shape; run on a GPU box:
    python tools/restrict_timing.py [taxa [trees]]          default 512 10000 (32-bit cells: the 34 GB table)
Counts once, then per kept-taxon count (taxa - 12 and taxa / 2, seeded random drop sets): prunes the reference tree, cuts
the table down (best of 3 calls; the map of a pruned tree is increasing = the monotone instance), scores it, counts the
pruned trees into a table of their own twice (the second call is the timed recount) and checks 1e5 lookups of the two tables
against each other. The yardstick beside it: qs_table_remap with the identity permutation at `taxa` (the same launch shape with
fully coalesced reads). Prints one JSON line. Effective bytes = one read + one write of the DESTINATION table."""
import json
import os
import sys
import time

import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quartetscores_amd import engine, flatten, native_ingest, newick  # noqa: E402

HBM_TBPS = 8.0
n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
m = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
ref_nw = native_ingest.synth_trees(n, 1, 2000).decode().strip()
text = native_ingest.synth_trees(n, m, 2001)
ref = flatten.flatten_reference(ref_nw)
batch, _ = native_ingest.ingest_text(ref_nw, text, want_ranges=False)
trees = [t for t in text.decode().split("\n") if t.strip()]


def wall(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


src = engine.Context(n, 32)
src.table_alloc()
hb = src.batch_upload(batch, with_nodes=False)
src.count_batch(hb)
src.sync()
full_recount_ms = wall(lambda: (src.count_batch(hb, engine.QS_ALGO_AUTO | engine.QS_COUNT_OVERWRITE), src.sync()))
src.batch_free(hb)

# the yardstick: the remap kernel with the identity permutation
same = engine.Context(n, 32)
same.table_alloc()
same.sync()
ident_ms = [wall(lambda: (same.table_remap(src, np.arange(n)), same.sync())) for _ in range(3)]
same.close()

rng = np.random.default_rng(2003)
out = {"tool": "restrict_timing", "taxa": n, "trees": m, "count_bits": 32, "table_bytes": src.table_bytes,
       "full_recount_ms": round(full_recount_ms, 2), "remap_identity_ms": round(min(ident_ms), 2),
       "remap_identity_ms_calls": [round(x, 2) for x in ident_ms],
       "remap_identity_effective_TBps": round(2 * src.table_bytes / (min(ident_ms) * 1e-3) / 1e12, 3), "kept": {}}
for kept in (n - 12, n // 2):
    drop = [ref.names[i] for i in rng.choice(n, size=n - kept, replace=False)]
    small_nw = newick.write(newick.prune(ref.root, drop))
    small = flatten.flatten_reference(small_nw)
    ids = flatten.taxon_restriction(small, ref)
    assert (np.diff(ids.astype(np.int64)) > 0).all()
    dst = engine.Context(kept, 32)
    dst.table_alloc()
    dst.sync()
    restrict_ms = [wall(lambda: (dst.table_restrict(src, ids), dst.sync())) for _ in range(3)]
    score_ms = [wall(lambda: dst.score(small)) for _ in range(2)]
    prune_s = time.perf_counter()
    small_text = "\n".join(native_ingest.prune_newick(t, drop) for t in trees).encode()
    prune_s = time.perf_counter() - prune_s
    small_batch, _ = native_ingest.ingest_text(small_nw, small_text, want_ranges=False)
    again = engine.Context(kept, 32)
    again.table_alloc()
    hs = again.batch_upload(small_batch, with_nodes=False)
    again.count_batch(hs)
    again.sync()
    recount_ms = wall(lambda: (again.count_batch(hs, engine.QS_ALGO_AUTO | engine.QS_COUNT_OVERWRITE), again.sync()))
    q = np.stack([rng.choice(kept, 4, replace=False) for _ in range(100000)])
    got = dst.lookup(q)
    lookups_match = bool((got == again.lookup(q)).all() and (got == src.lookup(ids.astype(np.int64)[q])).all() and got.sum() > 0)
    again.batch_free(hs)
    again.close()
    best = min(restrict_ms)
    tbps = 2 * dst.table_bytes / (best * 1e-3) / 1e12
    out["kept"][str(kept)] = {
        "table_bytes": dst.table_bytes, "table_share": round(dst.table_bytes / src.table_bytes, 3),
        "restrict_ms": round(best, 2), "restrict_ms_calls": [round(x, 2) for x in restrict_ms],
        "restrict_over_remap_identity": round(best / min(ident_ms), 3),
        "restrict_effective_TBps": round(tbps, 3), "restrict_hbm_roofline_frac": round(tbps / HBM_TBPS, 3),
        "score_ms": round(min(score_ms), 2), "restrict_plus_score_ms": round(best + min(score_ms), 2),
        "recount_pruned_ms": round(recount_ms, 2), "restrict_plus_score_over_recount": round((best + min(score_ms)) / recount_ms, 3),
        "host_prune_trees_s": round(prune_s, 2), "lookups_match": lookups_match,
    }
    dst.close()
out["box_issue_probe_ns_per_inst"] = round(src.issue_probe(), 4)
print(json.dumps(out))
