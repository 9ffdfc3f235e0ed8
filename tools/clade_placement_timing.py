"""qs_clade_placement beside the all-taxa qs_taxon_placement call, on configs[2]'s shape; run on a GPU box:
    python tools/clade_placement_timing.py [taxa [trees [out.json]]]          default 512 10000 (32-bit cells: the 34 GB table)
Counts the batch once, then times -- each best of 3 calls by the host clock around call + sync, downloads excluded -- the all-taxa
qs_taxon_placement call, qs_clade_placement over all eligible clades of the benchmark's reference tree, over the costliest single
clade and over one two-taxon clade, with the tuples each call gathers (the sum of |C| x C(n-|C|,3)). Checks the one-clade rows
against the all-clades call and every leaf row of a clade call against qs_taxon_placement, and prints one JSON line (also written
to out.json if given). The bar of DESIGN.md 13: ns per gathered tuple of the all-clades call <= 1.25 x that of the all-taxa call."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from quartetscores_amd import engine, flatten, native_ingest  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 512
m = int(args[1]) if len(args) > 1 else 10000
out_path = args[2] if len(args) > 2 else None
ref_nw = native_ingest.synth_trees(n, 1, 2000).decode().strip()
text = native_ingest.synth_trees(n, m, 2001)
ref = flatten.flatten_reference(ref_nw)
batch, _ = native_ingest.ingest_text(ref_nw, text, want_ranges=False)


def best_of_3(f):
    ms = []
    for _ in range(3):
        t = time.perf_counter()
        f()
        ctx.sync()
        ms.append((time.perf_counter() - t) * 1e3)
    return ms


ctx = engine.Context(n, 32)
ctx.table_alloc()
hb = ctx.batch_upload(batch, with_nodes=False)
ctx.count_batch(hb)
ctx.sync()
ctx.batch_free(hb)

_, _, lo, hi, _, _ = engine._tree_arrays(ref)
size = hi - lo
tuples = lambda v: int(size[v]) * ((n - int(size[v])) * (n - int(size[v]) - 1) * (n - int(size[v]) - 2) // 6)
nodes = engine.eligible_clades(ref)
costliest = int(max(nodes, key=tuples))
pair = int(next(v for v in nodes if size[v] == 2))
s, keep = ctx._ref_struct(ref)
width = 2 * ref.n_nodes
taxa_buf = torch.empty(n * width, dtype=torch.int64, device="cuda")
clade_buf = torch.empty(len(nodes) * width, dtype=torch.int64, device="cuda")
small_buf = torch.empty(n * width, dtype=torch.int64, device="cuda")


def place_taxa():
    ctx._chk(ctx.L.qs_taxon_placement(ctx.h, C.byref(s), None, n, C.c_void_p(taxa_buf.data_ptr())))


def place_clades(ids, buf):
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    ctx._chk(ctx.L.qs_clade_placement(ctx.h, C.byref(s), ids.ctypes.data_as(C.c_void_p), len(ids), C.c_void_p(buf.data_ptr())))
    return ids          # (lent for the call only; returned to keep the timing lambdas one expression)


place_taxa(); ctx.sync()              # warm: reference upload, link lookups, code objects
taxa_ms = best_of_3(place_taxa)
place_clades(nodes, clade_buf); ctx.sync()
all_ms = best_of_3(lambda: place_clades(nodes, clade_buf))
rows = clade_buf.cpu().numpy().reshape(len(nodes), width)
row_of = {int(v): i for i, v in enumerate(nodes)}
place_clades([costliest], small_buf); ctx.sync()
costliest_ms = best_of_3(lambda: place_clades([costliest], small_buf))
same = bool((small_buf[:width].cpu().numpy() == rows[row_of[costliest]]).all())
place_clades([pair], small_buf); ctx.sync()
pair_ms = best_of_3(lambda: place_clades([pair], small_buf))
same = same and bool((small_buf[:width].cpu().numpy() == rows[row_of[pair]]).all())
place_clades(ref.leaf_node, small_buf); ctx.sync()      # every leaf as a clade of one: the rows of the all-taxa call
leaves_ms = best_of_3(lambda: place_clades(ref.leaf_node, small_buf))
leaves_equal = bool((small_buf.cpu().numpy() == taxa_buf.cpu().numpy()).all())
cols = engine.clade_placement_columns(ref, nodes, engine.placement_scores(ref, rows))
table_bytes = ctx.table_bytes
probe = ctx.issue_probe()
ctx.close()

per_taxon = (n - 1) * (n - 2) * (n - 3) // 6
all_tuples = sum(tuples(v) for v in nodes)
ns = lambda ms, t: min(ms) * 1e6 / t
positions = int(np.mean([np.count_nonzero(~((lo >= lo[v]) & (hi <= hi[v]))) - 1 for v in nodes]))   # (without the root)
result = {
    "tool": "clade_placement_timing", "taxa": n, "trees": m, "count_bits": 32, "table_bytes": table_bytes,
    "taxa_all_ms": round(min(taxa_ms), 2), "taxa_all_ms_calls": [round(x, 2) for x in taxa_ms], "taxa_all_tuples": n * per_taxon,
    "clades_all_ms": round(min(all_ms), 2), "clades_all_ms_calls": [round(x, 2) for x in all_ms], "clades": len(nodes), "clades_all_tuples": all_tuples,
    "costliest_clade_ms": round(min(costliest_ms), 2), "costliest_clade_ms_calls": [round(x, 2) for x in costliest_ms],
    "costliest_clade_size": int(size[costliest]), "costliest_clade_tuples": tuples(costliest),
    "pair_clade_ms": round(min(pair_ms), 2), "pair_clade_ms_calls": [round(x, 2) for x in pair_ms], "pair_clade_tuples": tuples(pair),
    "leaves_as_clades_ms": round(min(leaves_ms), 2), "leaves_as_clades_ms_calls": [round(x, 2) for x in leaves_ms],
    "ns_per_tuple_taxa_all": round(ns(taxa_ms, n * per_taxon), 6), "ns_per_tuple_clades_all": round(ns(all_ms, all_tuples), 6),
    "ns_per_tuple_costliest": round(ns(costliest_ms, tuples(costliest)), 6), "ns_per_tuple_pair": round(ns(pair_ms, tuples(pair)), 6),
    "ns_per_tuple_leaves_as_clades": round(ns(leaves_ms, n * per_taxon), 6),
    "ratio_clades_to_taxa": round(ns(all_ms, all_tuples) / ns(taxa_ms, n * per_taxon), 4),
    "bar_ratio_le_1_25": bool(ns(all_ms, all_tuples) <= 1.25 * ns(taxa_ms, n * per_taxon)),
    "tuples_ratio_clades_to_taxa": round(all_tuples / (n * per_taxon), 3),
    "single_rows_equal_all_clades_call": same, "leaf_rows_equal_taxon_placement": leaves_equal,
    "clades_that_would_move": int((cols["gain"] > 0).sum()), "mean_edges_outside_a_clade": positions,
    "box_issue_probe_ns_per_inst": round(probe, 4),
}
line = json.dumps(result)
print(line)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write(line + "\n")
