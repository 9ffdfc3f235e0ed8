"""qs_taxon_placement beside a count pass and qs_taxon_support, on configs[2]'s shape; run on a GPU box:
    python tools/placement_timing.py [taxa [trees [out.json]]]          default 512 10000 (32-bit cells: the 34 GB table)
Counts the batch once, times a second count of the same batch (QS_COUNT_OVERWRITE, so the table stays one count; host clock around
call + sync), the per-taxon pass, the placement of one taxon (the middle id) and of all taxa -- each best of 3 calls by the host
clock around call + sync, downloads excluded --, checks the two identities with qs_taxon_support on every taxon, and prints one
JSON line (also written to out.json if given). The bars of DESIGN.md 12: all taxa <= the count pass, one taxon <= the per-taxon pass."""
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
width = 2 * ref.n_nodes
support_buf = torch.empty(6 * n, dtype=torch.int64, device="cuda")
links_buf = torch.empty(n * width, dtype=torch.int64, device="cuda")
one = np.array([n // 2], dtype=np.uint16)


def support():
    ctx._chk(ctx.L.qs_taxon_support(ctx.h, C.byref(s), C.c_void_p(support_buf.data_ptr())))


def place(ids):
    ctx._chk(ctx.L.qs_taxon_placement(ctx.h, C.byref(s), None if ids is None else ids.ctypes.data_as(C.c_void_p), n if ids is None else len(ids),
                                      C.c_void_p(links_buf.data_ptr())))


support(); ctx.sync()                 # warm: reference upload, plans, code objects
support_ms = best_of_3(support)
place(one); ctx.sync()
one_ms = best_of_3(lambda: place(one))
one_row = links_buf[:width].cpu().numpy().copy()
place(None); ctx.sync()
all_ms = best_of_3(lambda: place(None))
links = links_buf.cpu().numpy().reshape(n, width)
counts = support_buf.cpu().numpy().reshape(n, 6)
scores = engine.placement_scores(ref, links)
own = scores[np.arange(n), ref.leaf_node.astype(np.int64)]
identities = bool((own == counts[:, 1]).all() and (links.sum(axis=1) == counts[:, 1:4].sum(axis=1)).all() and (one_row == links[n // 2]).all())
cols = engine.placement_columns(ref, list(range(n)), scores)
table_bytes = ctx.table_bytes
probe = ctx.issue_probe()
ctx.close()

result = {
    "tool": "placement_timing", "taxa": n, "trees": m, "count_bits": 32, "table_bytes": table_bytes,
    "count_pass_ms": round(min(count_ms), 2), "count_pass_ms_calls": [round(x, 2) for x in count_ms],
    "taxon_support_ms": round(min(support_ms), 2), "taxon_support_ms_calls": [round(x, 2) for x in support_ms],
    "place_one_ms": round(min(one_ms), 2), "place_one_ms_calls": [round(x, 2) for x in one_ms],
    "place_all_ms": round(min(all_ms), 2), "place_all_ms_calls": [round(x, 2) for x in all_ms],
    "bar_all_le_count_pass": bool(min(all_ms) <= min(count_ms)), "bar_one_le_taxon_support": bool(min(one_ms) <= min(support_ms)),
    "tuples_per_taxon": (n - 1) * (n - 2) * (n - 3) // 6,
    "identities_hold": identities, "taxa_that_would_move": int((cols["gain"] > 0).sum()),
    "box_issue_probe_ns_per_inst": round(probe, 4),
}
line = json.dumps(result)
print(line)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write(line + "\n")
