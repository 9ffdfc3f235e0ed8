"""qs_branch_taxon_support beside qs_taxon_placement (the kernel yardstick) and beside the route it replaces, one qs_table_restrict +
qs_score per dropped taxon (the feature yardstick), on configs[2]'s shape; run on a GPU box:
    python tools/drop_one_timing.py [taxa [trees [out.json]]]             default 512 10000 (32-bit cells: the 34 GB table)
The two measurements are two child processes of this script, each under its own `timeout`, chained with `&&`, so that trouble in
the first ends the run; each counts the batch once, records qs_issue_probe and writes its part, and the parent merges the parts
into one JSON line (also written to out.json if given). Every figure is the best of 3 calls by the host clock around call + sync,
downloads excluded, the three values kept.
  kernel:  qs_branch_taxon_support for all taxa and for one (the middle id), rows alone (totals = NULL: the gather) and with the
           totals (one more streaming read), against qs_taxon_placement of the same lists, which reads the same tuples.
           Bar: the gather takes at most 2 x the placement's time.
  feature: for three seeded taxa, qs_table_restrict onto the other taxa plus qs_score (exact QP sums) of the pruned tree; their mean
           x taxa is what the matrix costs today. Bar: the new call for all taxa with totals costs at most a tenth of that."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

args = [a for a in sys.argv[1:] if not a.startswith("--")]
step = args.pop(0) if args and args[0] in ("kernel", "feature") else None
n = int(args[0]) if len(args) > 0 else 512
m = int(args[1]) if len(args) > 1 else 10000
out_path = args[2] if len(args) > 2 else None


def ms3(ms):
    return [round(x, 2) for x in ms]


def counted_context():
    from quartetscores_amd import engine, flatten, native_ingest
    ref_nw = native_ingest.synth_trees(n, 1, 2000).decode().strip()
    text = native_ingest.synth_trees(n, m, 2001)
    ref = flatten.flatten_reference(ref_nw)
    batch, _ = native_ingest.ingest_text(ref_nw, text, want_ranges=False)
    ctx = engine.Context(n, 32)
    ctx.table_alloc()
    hb = ctx.batch_upload(batch, with_nodes=False)
    ctx.count_batch(hb)
    ctx.sync()
    ctx.batch_free(hb)
    return engine, ctx, ref, ref_nw


def best_of_3(ctx, f):
    ms = []
    for _ in range(3):
        t = time.perf_counter()
        f()
        ctx.sync()
        ms.append((time.perf_counter() - t) * 1e3)
    return ms


def kernel_step():
    import numpy as np
    import torch
    engine, ctx, ref, _ = counted_context()
    N = ref.n_nodes
    s, keep = ctx._ref_struct(ref)
    links_buf = torch.empty(n * 2 * N, dtype=torch.int64, device="cuda")
    rows_buf = torch.empty((n + 1) * N * 4, dtype=torch.int64, device="cuda")
    one = np.array([n // 2], dtype=np.uint16)

    def place(ids):
        ctx._chk(ctx.L.qs_taxon_placement(ctx.h, C.byref(s), None if ids is None else ids.ctypes.data_as(C.c_void_p), n if ids is None else len(ids),
                                          C.c_void_p(links_buf.data_ptr())))

    def branch(ids, totals):
        k = n if ids is None else len(ids)
        ctx._chk(ctx.L.qs_branch_taxon_support(ctx.h, C.byref(s), None if ids is None else ids.ctypes.data_as(C.c_void_p), k, C.c_void_p(rows_buf.data_ptr()),
                                               C.c_void_p(rows_buf.data_ptr() + k * N * 4 * 8) if totals else None))

    out = {}
    for name, f in (("place_all", lambda: place(None)), ("place_one", lambda: place(one)),
                    ("rows_one", lambda: branch(one, False)), ("with_totals_one", lambda: branch(one, True)),
                    ("rows_all", lambda: branch(None, False)), ("with_totals_all", lambda: branch(None, True))):
        f(); ctx.sync()                   # warm: reference upload, plans, code objects
        if name == "with_totals_one":
            one_row = rows_buf[: N * 4].cpu().numpy().copy()
        ms = best_of_3(ctx, f)
        out[name + "_ms"], out[name + "_ms_calls"] = round(min(ms), 2), ms3(ms)
    host = rows_buf.cpu().numpy()
    rows, totals = host[: n * N * 4].reshape(n, N, 4), host[n * N * 4:].reshape(N, 4)
    out["rows_add_up_to_4_totals"] = bool((rows.sum(axis=0) == 4 * totals).all() and totals.any())
    out["one_row_equals_its_row_of_all"] = bool((one_row == rows[n // 2].reshape(-1)).all())
    cols = engine.drop_one_columns(ref, None, rows, totals)
    top = int(np.nanargmax(cols["delta"]))
    out["largest_delta"] = [int(cols["taxon"][top]), int(cols["node"][top]), round(float(cols["delta"][top]), 6)]
    out["rows_all_over_place_all"] = round(out["rows_all_ms"] / out["place_all_ms"], 3)
    out["rows_one_over_place_one"] = round(out["rows_one_ms"] / out["place_one_ms"], 3)
    out["with_totals_all_over_place_all"] = round(out["with_totals_all_ms"] / out["place_all_ms"], 3)
    out["with_totals_one_over_place_one"] = round(out["with_totals_one_ms"] / out["place_one_ms"], 3)
    out["bar_rows_le_2x_placement"] = bool(out["rows_all_over_place_all"] <= 2.0 and out["rows_one_over_place_one"] <= 2.0)
    out["table_bytes"] = ctx.table_bytes
    out["box_issue_probe_ns_per_inst"] = round(ctx.issue_probe(), 4)
    del keep
    ctx.close()
    return out


def feature_step():
    import numpy as np
    from quartetscores_amd import flatten, newick
    engine, ctx, ref, ref_nw = counted_context()
    dst = engine.Context(n - 1, 32)
    dst.table_alloc()
    picks = sorted(int(x) for x in np.random.default_rng(17).choice(n, size=3, replace=False))
    per_taxon, calls = [], []
    for x in picks:
        small = flatten.flatten_reference(newick.write(newick.prune(newick.parse_tree(ref_nw), [ref.names[x]])))
        ids = flatten.taxon_restriction(small, ref)

        def old_route():
            dst.table_restrict(ctx, ids)
            dst.score(small, engine.QS_SCORE_QP_EXACT64)

        old_route(); dst.sync()           # warm: this tree's upload and plans
        ms = best_of_3(dst, old_route)
        per_taxon.append(min(ms)); calls.append(ms3(ms))
    dst.close()
    ctx.branch_taxon_support(ref); ctx.sync()
    import torch
    N = ref.n_nodes
    s, keep = ctx._ref_struct(ref)
    buf = torch.empty((n + 1) * N * 4, dtype=torch.int64, device="cuda")
    new_ms = best_of_3(ctx, lambda: ctx._chk(ctx.L.qs_branch_taxon_support(ctx.h, C.byref(s), None, n, C.c_void_p(buf.data_ptr()),
                                                                          C.c_void_p(buf.data_ptr() + n * N * 4 * 8))))
    old_all = float(np.mean(per_taxon)) * n
    out = {"old_route_taxa": picks, "old_route_ms_per_taxon": ms3(per_taxon), "old_route_ms_calls": calls,
           "old_route_all_taxa_ms": round(old_all, 1), "new_call_all_taxa_ms": round(min(new_ms), 2), "new_call_all_taxa_ms_calls": ms3(new_ms),
           "new_over_old": round(min(new_ms) / old_all, 5), "bar_new_le_tenth_of_old": bool(min(new_ms) <= old_all / 10),
           "box_issue_probe_ns_per_inst": round(ctx.issue_probe(), 4)}
    del keep
    ctx.close()
    return out


if step:
    part = kernel_step() if step == "kernel" else feature_step()
    open(out_path, "w").write(json.dumps(part) + "\n")
    sys.exit(0)

tmp = tempfile.mkdtemp(prefix="drop_one_timing_")
parts = {k: os.path.join(tmp, f"drop_one_timing_{k}.part.json") for k in ("kernel", "feature")}
me = os.path.abspath(__file__)
chain = " && ".join(f"timeout -k 10 420 {sys.executable} {me} {k} {n} {m} {parts[k]}" for k in ("kernel", "feature"))
rc = subprocess.run(["bash", "-c", chain]).returncode
if rc != 0:
    sys.exit(f"drop_one_timing: a step ended with status {rc}; nothing written")
result = {"tool": "drop_one_timing", "taxa": n, "trees": m, "count_bits": 32, "tuples_per_taxon": (n - 1) * (n - 2) * (n - 3) // 6}
for k in ("kernel", "feature"):
    result[k] = json.load(open(parts[k]))
    os.remove(parts[k])
os.rmdir(tmp)
line = json.dumps(result)
print(line)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").write(line + "\n")
