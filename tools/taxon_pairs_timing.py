"""qs_taxon_pair_support beside a count pass, qs_taxon_support and qs_taxon_placement, on configs[2]'s shape; run on a GPU box:
    python tools/taxon_pairs_timing.py [taxa [trees [out.json]]]          default 512 10000 (32-bit cells: the 34 GB table)
Counts the batch once, times a second count of the same batch (QS_COUNT_OVERWRITE, so the table stays one count), the per-taxon
pass, the placement of all taxa, one row of the pair matrix (the middle id) and all rows -- each best of 3 calls by the host clock
around call + sync, downloads excluded, the three values kept --, checks the identities of DESIGN.md 16 with qs_taxon_support and
the symmetry on that table, and prints one JSON line (also written to out.json if given). The bars of DESIGN.md 16, both against
passes that this call did not change: all rows <= the count pass, one row <= the per-taxon pass."""
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
count_ms = best_of_3(lambda: ctx.count_batch(hb, engine.QS_ALGO_GATHER | engine.QS_COUNT_OVERWRITE))
ctx.batch_free(hb)

s, keep = ctx._ref_struct(ref)
support_buf = torch.empty(6 * n, dtype=torch.int64, device="cuda")
links_buf = torch.empty(n * 2 * ref.n_nodes, dtype=torch.int64, device="cuda")
pairs_buf = torch.empty(n * n * 8, dtype=torch.int64, device="cuda")
one = np.array([n // 2], dtype=np.uint16)


def support():
    ctx._chk(ctx.L.qs_taxon_support(ctx.h, C.byref(s), C.c_void_p(support_buf.data_ptr())))


def place():
    ctx._chk(ctx.L.qs_taxon_placement(ctx.h, C.byref(s), None, n, C.c_void_p(links_buf.data_ptr())))


def pairs(ids):
    ctx._chk(ctx.L.qs_taxon_pair_support(ctx.h, C.byref(s), None if ids is None else ids.ctypes.data_as(C.c_void_p), n if ids is None else len(ids),
                                         C.c_void_p(pairs_buf.data_ptr())))


def ms3(ms):
    return [round(x, 2) for x in ms]


support(); ctx.sync()                 # warm: reference upload, plans, code objects
support_ms = best_of_3(support)
place(); ctx.sync()
place_ms = best_of_3(place)
pairs(one); ctx.sync()
one_ms = best_of_3(lambda: pairs(one))
one_row = pairs_buf[: n * 8].cpu().numpy().copy()
pairs(None); ctx.sync()
all_ms = best_of_3(lambda: pairs(None))
matrix = pairs_buf.cpu().numpy().reshape(n, n, 8)
counts = support_buf.cpu().numpy().reshape(n, 6)
row = matrix.sum(axis=1)
resolved, conc, disc, eval_only = (counts[:, k] for k in range(4))
symmetric = bool((matrix == matrix.transpose(1, 0, 2)).all() and not matrix[np.arange(n), np.arange(n)].any())
identities = bool((row[:, 0] == resolved).all() and (row[:, 1] == 2 * resolved).all() and (row[:, 2] == conc).all() and
                  (row[:, 4] == disc).all() and (row[:, 6] - row[:, 2] - row[:, 4] == eval_only).all() and
                  (row[:, 7] == 3 * (conc + disc + eval_only)).all() and (row[:, 3] == conc + disc).all() and
                  (one_row == matrix[n // 2].reshape(-1)).all())
cols = engine.taxon_pair_columns(matrix, ref.names)
apart = cols["ref_apart"] > 0
top = int(np.nanargmax(np.where(apart, cols["joined"], np.nan))) if apart.any() else -1
table_bytes = ctx.table_bytes
probe = ctx.issue_probe()
ctx.close()

result = {
    "tool": "taxon_pairs_timing", "taxa": n, "trees": m, "count_bits": 32, "table_bytes": table_bytes,
    "count_pass_ms": round(min(count_ms), 2), "count_pass_ms_calls": ms3(count_ms),
    "taxon_support_ms": round(min(support_ms), 2), "taxon_support_ms_calls": ms3(support_ms),
    "place_all_ms": round(min(place_ms), 2), "place_all_ms_calls": ms3(place_ms),
    "pairs_one_ms": round(min(one_ms), 2), "pairs_one_ms_calls": ms3(one_ms),
    "pairs_all_ms": round(min(all_ms), 2), "pairs_all_ms_calls": ms3(all_ms),
    "pairs_all_over_count_pass": round(min(all_ms) / min(count_ms), 4), "pairs_one_over_taxon_support": round(min(one_ms) / min(support_ms), 4),
    "pairs_all_over_place_all": round(min(all_ms) / min(place_ms), 3),
    "bar_all_le_count_pass": bool(min(all_ms) <= min(count_ms)), "bar_one_le_taxon_support": bool(min(one_ms) <= min(support_ms)),
    "tuples_per_taxon": (n - 1) * (n - 2) * (n - 3) // 6,
    "identities_hold": identities, "symmetric": symmetric,
    "largest_joined": None if top < 0 else [int(cols["a"][top]), int(cols["b"][top]), round(float(cols["joined"][top]), 6)],
    "box_issue_probe_ns_per_inst": round(probe, 4),
}
line = json.dumps(result)
print(line)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write(line + "\n")
