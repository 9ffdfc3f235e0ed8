"""Every output option of QuartetScores that needs something of the run, without a GPU: FILE that exists, FILE that is the -q file
as well, and a run that does not offer what the option's class needs are refused before the device is touched -- exit status 1, the
message that names the flag, no [trace] line and no output file."""
import os
import subprocess

import pytest

from quartetscores_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "quartetscores_amd", "bin", "QuartetScores")
N = 8

WHOLE_TABLE = "needs the whole count table on one GPU: omit --gpus / --table-shards"
COUNTED_TREES = "needs the evaluation trees counted on one GPU: omit --gpus / --table-shards / --load-table"
# flag -> (the arguments in front of FILE, the class's message, the run switches that refuse the class)
SPLIT = [["--gpus", "2"], ["--table-shards", "2"]]
OUTPUTS = {
    "--per-taxon": ([], WHOLE_TABLE, SPLIT),
    "--place-taxa": ([], WHOLE_TABLE, SPLIT),
    "--place-clades": ([], WHOLE_TABLE, SPLIT),
    "--test-groups": (["groups.txt"], WHOLE_TABLE, SPLIT),
    "--taxon-pairs": ([], WHOLE_TABLE, SPLIT),
    "--drop-one": ([], WHOLE_TABLE, SPLIT),
    "--per-tree": ([], COUNTED_TREES, SPLIT + [["--load-table", "table.bin"]]),
    "--tree-distances": ([], COUNTED_TREES, SPLIT + [["--load-table", "table.bin"]]),
    "--branch-trees": ([], COUNTED_TREES, SPLIT + [["--load-table", "table.bin"]]),
    "--bootstrap": ([], COUNTED_TREES, SPLIT + [["--load-table", "table.bin"]]),
    "--local-pp": ([], COUNTED_TREES, SPLIT + [["--load-table", "table.bin"]]),
}
INPUTS = ("r.nwk", "e.nwk", "groups.txt", "table.bin")


@pytest.fixture()
def files(tmp_path):
    (tmp_path / "r.nwk").write_text(synth.reference_tree(N, 1) + "\n")
    (tmp_path / "e.nwk").write_text("\n".join(synth.tree_set(N, 6, 2)) + "\n")
    (tmp_path / "groups.txt").write_text("h\tt0,t1\tt2,t3\n")
    (tmp_path / "table.bin").write_bytes(b"never read")
    return tmp_path


def run(files, flag, path, *extra):
    before = [str(files / name) for name in OUTPUTS[flag][0]]
    args = ["-r", files / "r.nwk", "-e", files / "e.nwk", "-o", files / "o.nwk", flag, *before, path, *extra, "--trace"]
    return subprocess.run([BIN, *map(str, args)], capture_output=True, text=True, timeout=600)


def refused(p, files, *message, kept=()):
    assert p.returncode == 1 and all(part in p.stderr for part in message), p.stderr
    assert "[trace]" not in p.stderr
    assert sorted(os.listdir(files)) == sorted(INPUTS + tuple(kept))


@pytest.mark.parametrize("flag", OUTPUTS)
def test_refused_existing_file(files, flag):
    (files / "f.tsv").write_text("keep\n")
    p = run(files, flag, files / "f.tsv")
    refused(p, files, f"{flag}: the output file {files / 'f.tsv'} already exists", kept=("f.tsv",))
    assert (files / "f.tsv").read_text() == "keep\n"


@pytest.mark.parametrize("flag", OUTPUTS)
def test_refused_file_that_is_the_qic_file(files, flag):
    p = run(files, flag, files / "shared.out", "-q", files / "shared.out")
    refused(p, files, f"{flag}: {files / 'shared.out'} is also another output file")


@pytest.mark.parametrize("flag,extra", [(flag, extra) for flag, (_, _, switches) in OUTPUTS.items() for extra in switches],
                         ids=lambda v: v if isinstance(v, str) else v[0])
def test_refused_where_the_run_lacks_what_the_class_needs(files, flag, extra):
    extra = [str(files / x) if x == "table.bin" else x for x in extra]
    p = run(files, flag, files / "f.tsv", *extra)
    refused(p, files, f"{flag} {OUTPUTS[flag][1]}")
