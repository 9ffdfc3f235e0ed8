"""qs_table_collapse beside a plain read of the source tuples it must read and beside the only other route (one qs_group_support quad
hypothesis per 4-set of species); run on a GPU box:
    python tools/species_map_timing.py [out.json [read_bw_output.txt]]      default profiles/r21_species_map_timing.json
Shapes: 512 individuals x 10 000 binary trees (configs[2]'s table, 32-bit cells) collapsed to 128 species of 4 and to 449 species (one
of 64 individuals, the rest singletons: the load-imbalance case), and 128 individuals collapsed to 32 species. Per shape: the time of
qs_table_collapse alone (HIP events around the call on the null stream both contexts use: the 8 KB upload of the id lists is inside;
best of 3 after a warm call), the bytes of the source tuples with four different species (exact, from first_id), the time of a torch
int32 reduction over that many bytes at the head of the SAME buffer (tools/bw_probe.py's probe, best of 4: it stays under 1 TB/s and
is no roof, so no ratio to it is written); a check of 300 seeded destination tuples against sums of qs_lookup over the individuals. For
the first shape also the other route: C(128,4) hypotheses x the per-hypothesis time of qs_group_support (64 quad hypotheses = 8 reads
of the table), and the wall time the CLI adds: QuartetScores on the same trees with --species-map (128 species) and without
(the 512 leaves as taxa). read_bw_output.txt: the output of tools/bin/read_bw (a 32 GB buffer of its own) from the same job; its best rate is recorded, and per
shape the time of the needed bytes at that rate and the collapse's ratio to it -- the yardstick to quote. read_bw does not read the table's own buffer: a
plain read of the same buffer by that probe is not built."""
import itertools
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quartetscores_amd import engine, native_ingest  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r21_species_map_timing.json")
read_bw_path = sys.argv[2] if len(sys.argv) > 2 else None
BIN = os.path.join(ROOT, "quartetscores_amd", "bin", "QuartetScores")
M = 10000


def distinct_species_4sets(sizes):
    """the number of 4-sets of individuals with four different species: the elementary symmetric polynomial e4 of the group sizes"""
    e = [1, 0, 0, 0, 0]
    for s in sizes:
        for k in (4, 3, 2, 1):
            e[k] += e[k - 1] * int(s)
    return e[4]


def counted(n, bits):
    """n individuals t0 .. t{n-1} in id order (a star tree as the flattening's reference), M random binary trees, counted into a torch buffer"""
    star = "(" + ",".join(f"t{i}" for i in range(n)) + ");"
    text = native_ingest.synth_trees(n, M, 2101)
    batch, _ = native_ingest.ingest_text(star, text, want_ranges=False)
    ctx = engine.Context(n, bits)
    buf = torch.zeros((ctx.table_bytes + 16 + 3) // 4, dtype=torch.int32, device="cuda")
    ctx.table_attach(buf)
    ctx.table_clear()
    hb = ctx.batch_upload(batch, with_nodes=False)
    ctx.count_batch(hb)
    ctx.sync()
    ctx.batch_free(hb)
    return ctx, buf, text


def plain_read_ms(buf, nbytes):
    head = buf[: (nbytes + 3) // 4]
    best = 1e9
    for _ in range(4):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); head.sum(); b.record(); b.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def collapse_case(src, buf, sizes, dst_bits, rng):
    n_src, n_dst = int(np.sum(sizes)), len(sizes)
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint16)
    dst = engine.Context(n_dst, dst_bits)
    dst.table_alloc()
    dst.table_collapse(src, first); dst.sync()          # warm: code object, id buffers
    ms = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); dst.table_collapse(src, first); b.record(); b.synchronize()
        dst.sync()
        ms.append(a.elapsed_time(b))
    cell = src.count_bits // 8
    need = distinct_species_4sets(sizes) * 3 * cell
    read_ms = plain_read_ms(buf, need)
    # spot check: seeded destination tuples against the sums of lookups over one individual per species
    quads = np.sort(np.stack([rng.choice(n_dst, 4, replace=False) for _ in range(300)]), axis=1)
    got = dst.lookup(quads.astype(np.uint16))
    ok = True
    for q, g in zip(quads, got):
        combos = np.array(list(itertools.product(*(range(first[s], first[s + 1]) for s in q))), dtype=np.uint16)
        ok = ok and bool((src.lookup(combos).sum(axis=0) == g).all())
    res = {"individuals": n_src, "species": n_dst, "largest_group": int(max(sizes)), "src_bits": src.count_bits, "dst_bits": dst_bits,
           "src_table_bytes": src.table_bytes, "dst_table_bytes": dst.table_bytes,
           "source_bytes_needed": need, "source_share_needed": round(need / src.table_bytes, 4),
           "collapse_ms": round(min(ms), 3), "collapse_ms_calls": [round(x, 3) for x in ms],
           "collapse_effective_TBps": round(need / (min(ms) * 1e-3) / 1e12, 3),
           "torch_reduction_ms": round(read_ms, 3), "torch_reduction_TBps": round(need / (read_ms * 1e-3) / 1e12, 3), "spot_check_300_tuples_match": ok, "dst_nonzero": bool(got.sum() > 0)}
    return res, dst


rng = np.random.default_rng(2102)
out = {"tool": "species_map_timing", "trees": M, "cases": {}}
src, buf, text512 = counted(512, 32)
res, dst = collapse_case(src, buf, [4] * 128, 32, rng)
out["cases"]["512_to_128_by_4"] = res

# the only other route: one quad hypothesis per 4-set of species
labels = np.zeros((64, 512), dtype=np.uint8)
for h in range(64):
    for k, s in enumerate(rng.choice(128, 4, replace=False), 1):
        labels[h, 4 * s:4 * s + 4] = k
src.group_support(labels)
t = []
for _ in range(3):
    t0 = time.perf_counter(); src.group_support(labels); t.append((time.perf_counter() - t0) * 1e3)
per_hyp = min(t) / 64
n_sets = 128 * 127 * 126 * 125 // 24
out["other_route"] = {"group_support_ms_per_hypothesis_at_64": round(per_hyp, 3), "species_4sets": n_sets,
                      "hours": round(n_sets * per_hyp / 3.6e6, 2), "over_collapse": round(n_sets * per_hyp / res["collapse_ms"], 0)}
dst.close()
res, dst = collapse_case(src, buf, [1] * 200 + [64] + [1] * 248, 32, rng)
out["cases"]["512_to_449_one_of_64"] = res
dst.close()
out["box_issue_probe_ns_per_inst"] = round(src.issue_probe(), 4)
src.close()
del buf
torch.cuda.empty_cache()
src, buf, _ = counted(128, 16)
res, dst = collapse_case(src, buf, [4] * 32, 32, rng)
out["cases"]["128_to_32_by_4"] = res
dst.close(); src.close()
del buf
torch.cuda.empty_cache()

# the CLI: the same trees with the map (128 species) and without (512 taxa)
with tempfile.TemporaryDirectory() as tmp:
    species_nw = native_ingest.synth_trees(128, 1, 2103).decode().strip()
    from quartetscores_amd import flatten  # noqa: E402
    names = flatten.flatten_reference(species_nw).names
    p = lambda x: os.path.join(tmp, x)
    open(p("species.nwk"), "w").write(species_nw + "\n")
    open(p("taxa.nwk"), "w").write(native_ingest.synth_trees(512, 1, 2104).decode().strip() + "\n")
    open(p("e.nwk"), "wb").write(text512)
    open(p("map.txt"), "w").write("".join(f"{s}:" + ",".join(f"t{4 * i + j}" for j in range(4)) + "\n" for i, s in enumerate(names)))
    runs = {}
    for name, extra in (("plain_512_taxa", ["-r", p("taxa.nwk")]), ("species_map_128", ["-r", p("species.nwk"), "--species-map", p("map.txt")])):
        walls, collapsed = [], []
        for k in range(2):
            t0 = time.perf_counter()
            r = subprocess.run([BIN, "-e", p("e.nwk"), "-o", p(f"{name}{k}.out"), *extra], capture_output=True, text=True, timeout=300)
            walls.append(time.perf_counter() - t0)
            assert r.returncode == 0, r.stderr
            collapsed += [int(x) for x in re.findall(r"Collapsed the count table in (\d+) microseconds", r.stdout)]
        runs[name] = {"wall_s": [round(x, 3) for x in walls], "collapsed_us": collapsed}
    out["cli"] = runs
    out["cli"]["added_wall_s"] = round(min(runs["species_map_128"]["wall_s"]) - min(runs["plain_512_taxa"]["wall_s"]), 3)
if read_bw_path and os.path.exists(read_bw_path):
    figs = [float(x) for x in re.findall(r"(\d+\.\d+)(?=\s|$)", " ".join(l.split(":", 1)[1] for l in open(read_bw_path) if l.startswith("threads")))]
    out["read_bw_best_TBps"] = max(figs) if figs else None
    for case in out["cases"].values():   # the same bytes at the best rate of the streaming probe on this box
        if figs:
            case["read_bw_ms"] = round(case["source_bytes_needed"] / (max(figs) * 1e9), 3)
            case["collapse_over_read_bw"] = round(case["collapse_ms"] / case["read_bw_ms"], 2)
line = json.dumps(out)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(line + "\n")
