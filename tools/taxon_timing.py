"""qs_taxon_support beside pass 1 of qs_score and a bare read of the table, on configs[2]'s shape; run on a GPU box:
    python tools/taxon_timing.py [taxa [trees [--cli]]]          default 512 10000 (32-bit cells: the 34 GB table)
Counts once, scores (qs_last_score_ms: pass 1 is the same bytes in the same row order), runs the per-taxon pass (best of 3
calls, host clock around call + sync), checks the identities against the score's node-pair sums cheaply (column sums), runs
tools/bin/read_bw (if built: hipcc -O3 --offload-arch=gfx950 -o tools/bin/read_bw tools/read_bw.hip) for the bare read, and
prints one JSON line. --cli: also the wall time of QuartetScores on the same trees with and without --per-taxon."""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quartetscores_amd import engine, flatten, native_ingest  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 512
m = int(args[1]) if len(args) > 1 else 10000
ref_nw = native_ingest.synth_trees(n, 1, 2000).decode().strip()
text = native_ingest.synth_trees(n, m, 2001)
ref = flatten.flatten_reference(ref_nw)
batch, _ = native_ingest.ingest_text(ref_nw, text, want_ranges=False)


def wall(f):
    t = time.perf_counter()
    r = f()
    return (time.perf_counter() - t) * 1e3, r


ctx = engine.Context(n, 32)
ctx.table_alloc()
hb = ctx.batch_upload(batch, with_nodes=False)
ctx.count_batch(hb)
ctx.sync()
ctx.batch_free(hb)
ctx.score(ref)                       # warm: reference upload, plans, code objects
pass1, score_total = [], []
for _ in range(3):
    t, _r = wall(lambda: ctx.score(ref))
    score_total.append(t)
    pass1.append(ctx.last_score_ms()["pass1"])
counts = ctx.taxon_support(ref)      # warm
taxon_ms = []
for _ in range(3):
    t, again = wall(lambda: ctx.taxon_support(ref))
    taxon_ms.append(t)
    assert (again == counts).all()
cols = engine.taxon_columns(counts)
quartets = n * (n - 1) * (n - 2) * (n - 3) // 24
# a binary reference resolves every quartet, and every tree of this set holds all taxa and is binary: every tuple sums to m
identities = bool(int(counts[:, 0].sum()) == 4 * quartets and int((counts[:, 1] + counts[:, 2]).sum()) == 4 * quartets * m
                  and int(counts[:, 3].sum()) == 0 and (counts[:, 4] + counts[:, 5] <= counts[:, 0]).all())
table_bytes = ctx.table_bytes
probe = ctx.issue_probe()
ctx.close()

bare_tbps = None
read_bw = os.path.join(ROOT, "tools", "bin", "read_bw")
if os.path.exists(read_bw):
    out = subprocess.run([read_bw, str(max(1, table_bytes >> 30))], capture_output=True, text=True, timeout=300).stdout
    vals = [float(x) for ln in out.splitlines() if ln.startswith("threads") for x in re.findall(r"(?:U=\d(?: nt)?) ([0-9.]+)", ln)]
    bare_tbps = max(vals) if vals else None

cli = None
if "--cli" in sys.argv:
    exe = os.path.join(ROOT, "quartetscores_amd", "bin", "QuartetScores")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "r.nwk"), "w").write(ref_nw + "\n")
        open(os.path.join(d, "e.nwk"), "wb").write(text)
        common = [exe, "-r", os.path.join(d, "r.nwk"), "-e", os.path.join(d, "e.nwk")]
        runs = {"plain": [], "per_taxon": []}
        for i in range(2):
            for kind in runs:
                extra = ["--per-taxon", os.path.join(d, f"p{i}.tsv")] if kind == "per_taxon" else []
                t, p = wall(lambda: subprocess.run(common + ["-o", os.path.join(d, f"{kind}{i}.nwk")] + extra, capture_output=True, timeout=600))
                assert p.returncode == 0, p.stderr
                runs[kind].append(t)
        same = open(os.path.join(d, "plain0.nwk"), "rb").read() == open(os.path.join(d, "per_taxon0.nwk"), "rb").read()
        cli = {"wall_ms_plain": round(min(runs["plain"]), 1), "wall_ms_per_taxon": round(min(runs["per_taxon"]), 1), "annotated_tree_identical": same}

best, p1 = min(taxon_ms), min(pass1)
print(json.dumps({
    "tool": "taxon_timing", "taxa": n, "trees": m, "count_bits": 32, "table_bytes": table_bytes,
    "taxon_ms": round(best, 2), "taxon_ms_calls": [round(x, 2) for x in taxon_ms],
    "score_pass1_ms": round(p1, 2), "score_pass1_ms_calls": [round(x, 2) for x in pass1], "score_total_ms": round(min(score_total), 2),
    "taxon_over_pass1": round(best / p1, 3), "bar_taxon_le_2x_pass1": bool(best <= 2 * p1),
    "taxon_effective_TBps": round(table_bytes / (best * 1e-3) / 1e12, 3), "pass1_effective_TBps": round(table_bytes / (p1 * 1e-3) / 1e12, 3),
    "bare_read_TBps": bare_tbps, "bare_read_ms": round(table_bytes / bare_tbps / 1e9, 2) if bare_tbps else None,
    "identities_hold": identities, "lowest_concordance_taxon": int(np.nanargmin(cols["concordance"])),
    "cli": cli, "box_issue_probe_ns_per_inst": round(probe, 4),
}))
