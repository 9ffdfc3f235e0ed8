"""Writes tests/golden/species_map_plain.json: what a QuartetScores binary writes for the plain (no --species-map) run of
tests/test_gpu_cli_species_map.py -- run with the binary of the commit BEFORE --species-map existed, so that the test can hold
the current binary's plain run against it byte for byte.

    python tests/golden/make_species_map_fixture.py /path/to/QuartetScores [out.json]      (needs a GPU)
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))

PLAIN_OUTPUTS = {"-o": "o.nwk", "-q": "q.txt", "--per-taxon": "taxon.tsv", "--place-taxa": "place.tsv", "--drop-one": "drop.tsv"}


def plain_inputs():
    """(reference tree, evaluation trees) of the plain run: the 8 species and 60 mixed trees over them"""
    from quartetscores_amd import synth
    n = 8
    trees = (synth.tree_set(n, 15, 212, dropout=0.2) + synth.tree_set(n, 15, 213, collapse=0.3) +
             synth.tree_set(n, 15, 214, rooted=True) + synth.tree_set(n, 15, 215))
    return synth.reference_tree(n, 211), trees


def run_plain(binary, folder):
    """the plain run with every output of PLAIN_OUTPUTS in `folder` -> {flag: text}"""
    ref, trees = plain_inputs()
    with open(os.path.join(folder, "r.nwk"), "w") as f:
        f.write(ref + "\n")
    with open(os.path.join(folder, "e.nwk"), "w") as f:
        f.write("\n".join(trees) + "\n")
    args = [binary, "-r", os.path.join(folder, "r.nwk"), "-e", os.path.join(folder, "e.nwk")]
    for flag, name in PLAIN_OUTPUTS.items():
        args += [flag, os.path.join(folder, name)]
    p = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    out = {}
    for flag, name in PLAIN_OUTPUTS.items():
        with open(os.path.join(folder, name)) as f:
            out[flag] = f.read()
    return out


if __name__ == "__main__":
    target = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "species_map_plain.json")
    with tempfile.TemporaryDirectory() as tmp:
        result = run_plain(sys.argv[1], tmp)
    with open(target, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", target, {k: len(v) for k, v in result.items()})
