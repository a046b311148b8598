#!/usr/bin/env python3
"""A transcript of the `sufr` CLI on the golden files, to compare two builds byte for byte.

    cli_transcript.py BINARY OUTFILE [--legs host,device] [--device ID] [--timeout SECONDS]
    cli_transcript.py --compare A B

A fixed list of invocations (rows() below) runs one process each, in order, on tests/golden/expected.  OUTFILE gets, per row,
the argv, the exit status, standard output, standard error and the sha256 of every file the row wrote (-o, --occ, --unique),
with the golden directory and the row's scratch directory replaced by <GOLDEN> and <TMP>.  The `host` leg runs the rows as
listed; the `device` leg appends `--device ID` to every row whose sub-command takes it.  The run ends at the first row that
dies of a signal or runs into its time limit (exit status 3): nothing is started on a device after a fault.

A sanitizer build's reports carry addresses and process ids; they are cut out of the recorded stderr and only their SUMMARY
lines are kept (`sanitizer:`).  --compare lists the rows that differ and tells those that differ only by a sanitizer summary
the first transcript has and the second has not; its exit status is 0 when no other difference exists."""
from __future__ import annotations

import hashlib
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "expected"
G, T = "<GOLDEN>", "<TMP>"
TAKES_DEVICE = {"count", "co", "locate", "lo", "extract", "ex", "match", "ma", "mems", "me", "approx", "ap", "edit", "ed",
                "kmers", "km", "repeats", "rp", "shared", "lz"}
ALL_FILES = ("1.sufr", "1n.sufr", "1s.sufr", "2.sufr", "2d.sufr", "2n.sufr", "2ns.sufr", "2s.sufr", "3.sufr", "abba.sufr",
             "long_dna_sequence.sufr", "long_dna_sequence_allow_ambiguity.sufr", "uniprot-masked.sufr", "uniprot.sufr")


def rows():
    r = []
    add = lambda *a: r.append([str(x) for x in a])
    uni, masked, dna, one, three = f"{G}/uniprot.sufr", f"{G}/uniprot-masked.sufr", f"{G}/long_dna_sequence.sufr", f"{G}/1.sufr", f"{G}/3.sufr"
    # -- kmers ---------------------------------------------------------------------------------------------------------
    add("kmers", "-k", 4, uni)                                                      # neither side file
    add("km", "-k", 3, one)
    add("kmers", "-k", 3, "-b", 2, one)
    add("kmers", "-k", 3, "--bins", 1, one)
    add("kmers", "-k", 4, "--occ", f"{T}/occ", uni)
    add("kmers", "-k", 4, "--unique", f"{T}/uniq", uni)
    add("kmers", "-k", 4, "--occ", f"{T}/occ", "--unique", f"{T}/uniq", uni)
    add("kmers", "-k", 4, "-b", 16, "--occ", f"{T}/occ", "--unique", f"{T}/uniq", "-o", f"{T}/out", uni)
    add("kmers", "-k", 11, "--occ", f"{T}/occ", "--unique", f"{T}/uniq", "--output", f"{T}/out", dna)
    for name in ALL_FILES:
        add("kmers", "-k", 2, "--occ", f"{T}/occ", "--unique", f"{T}/uniq", f"{G}/{name}")
    add("kmers", "-k", 3, masked)
    add("kmers", "-k", 3, "-o", f"{T}/out", masked)
    add("kmers", "-k", 0, one)
    add("kmers", "-k", 3, "-b", 0, one)
    add("kmers", one)
    add("kmers", "-k", 3)
    add("kmers", one, "-k")
    add("kmers", "-k", 3, "-t", 2, one)
    add("kmers", "-k", 3, one, one)
    add("kmers", "-k", 3, f"{G}/no-such-file.sufr")
    add("kmers", "-k", 3, "-o", f"{T}/no-such-dir/out", one)
    add("kmers", "-k", 3, "--occ", f"{T}/no-such-dir/occ", one)
    # -- repeats -------------------------------------------------------------------------------------------------------
    for kind in ("branching", "maximal", "super", "supermaximal"):
        add("repeats", "-l", 2, "--kind", kind, three)
    add("repeats", "-l", 2, three)
    add("rp", "-l", 1, "-c", 3, "-C", 9, "--max-positions", 2, "-o", f"{T}/out", three)
    add("repeats", "--min-len", 1, "--min-count", 3, "--max-count", 9, "--output", f"{T}/out", three)
    add("repeats", "-l", 1, "--kind", "super", "--max-positions", 0, three)
    add("repeats", "-l", 1, "--max-positions", 1, three)
    add("repeats", "-l", 6, "--kind", "maximal", uni)
    add("repeats", "-l", 9, "-c", 2, "-C", 5, dna)
    add("repeats", "-l", 100000, uni)                                               # no record
    add("repeats", "-l", 100000, "-o", f"{T}/out", uni)
    for name in ALL_FILES:
        add("repeats", "-l", 2, "--kind", "maximal", f"{G}/{name}")
    add("repeats", "-l", 3, "-o", f"{T}/out", masked)
    add("repeats", three)
    add("repeats", "-l", 3)
    add("repeats", "-l", 3, "--kind", "bogus", three)
    add("repeats", "-l", 3, "--kind")
    add("repeats", three, "-l")
    add("repeats", "-l", 3, "-t", 2, three)
    add("repeats", "-l", 3, "-q", 2, three)
    add("repeats", "-l", 3, f"{G}/no-such-file.sufr")
    add("repeats", "-l", 3, "-o", f"{T}/no-such-dir/out", three)
    # -- shared --------------------------------------------------------------------------------------------------------
    for name in ("2.sufr", "3.sufr", "uniprot.sufr"):
        add("shared", "--common", f"{G}/{name}")
        add("shared", "-q", 2, "-l", 3, f"{G}/{name}")
    for kind in ("branching", "maximal", "super", "supermaximal"):
        add("shared", "-l", 1, "-c", 2, "-C", 9, "--min-seqs", 1, "--max-seqs", 2, "--kind", kind, "--max-positions", 2, "-o", f"{T}/out", three)
    add("shared", "-l", 2, three)
    add("shared", "--min-len", 2, "--min-count", 3, "--max-count", 0, three)
    add("shared", "-l", 1, "--max-seqs", 1, "--max-positions", 0, three)
    add("shared", "--common", "-o", f"{T}/out", three)
    add("shared", "--common", "-l", 3, "--kind", "super", three)
    add("shared", "-l", 100000, "-q", 2, uni)                                        # no record
    for name in ALL_FILES:
        add("shared", "-l", 2, f"{G}/{name}")
        add("shared", "--common", f"{G}/{name}")
    add("shared", "-l", 3, "-o", f"{T}/out", masked)
    add("shared", "--common", "-o", f"{T}/out", masked)
    add("shared", three)
    add("shared", "-l", 3)
    add("shared", "-l", 3, "--kind", "bogus", three)
    add("shared", "-l", 3, "--min-seqs", 3, "--max-seqs", 2, three)
    add("shared", "-l", 3, "--min-seq", 2, three)
    add("shared", "-l", 3, "-q")
    add("shared", "-l", 3, "-t", 2, three)
    add("shared", "-l", 3, f"{G}/no-such-file.sufr")
    add("shared", "-l", 3, "-o", f"{T}/no-such-dir/out", three)
    add("shared", "--common", "-o", f"{T}/no-such-dir/out", three)
    # -- lz ------------------------------------------------------------------------------------------------------------
    for name in ALL_FILES:
        add("lz", f"{G}/{name}")
    add("lz", "--lpf", three)
    add("lz", "--lpf", one)
    add("lz", "--lpf", "-o", f"{T}/out", dna)
    add("lz", "-o", f"{T}/out", uni)
    add("lz", "-t", 2, uni)
    add("lz", "--threads", 1, "--lpf", three)
    add("lz", "--lpf", "-o", f"{T}/out", masked)
    add("lz")
    add("lz", "-t")
    add("lz", "--kind", "super", three)
    add("lz", three, three)
    add("lz", f"{G}/no-such-file.sufr")
    add("lz", "-o", f"{T}/no-such-dir/out", three)
    add("lz", "--lpf", "-o", f"{T}/no-such-dir/out", three)
    # -- the query commands: search_all and QuerySession hold the same device object ---------------------------------------
    add("count", one, "AC", "GT", "X")
    add("co", uni, "RNELNNEEA", "MSF", "ZZZZ")
    add("count", masked, "RNELNNEEA")
    add("count", "-o", f"{T}/out", dna, "ACGT", "GGGG")
    add("locate", one, "AC", "X")
    add("locate", "-a", uni, "RNELNNEEA", "MSF")
    add("locate", "-m", 3, dna, "ACGTAC")
    add("extract", "-p", 2, "-s", 5, one, "CG", "X")
    add("extract", uni, "RNELNNEEA")
    add("count", f"{G}/no-such-file.sufr", "AC")
    add("count", "-o", f"{T}/no-such-dir/out", one, "AC")
    add("count", one)
    add("count", one, "-m")
    add("match", "-k", 3, one, "ACGTA", "GTNNA", "XX")
    add("match", "-k", 3, "-n", 1, "-a", one, "ACGTA")
    add("match", "-k", 3, masked, "RNELNNEEA")
    add("match", "-k", 0, one, "ACGT")
    add("mems", "-k", 3, "-b", one, "ACGTA")
    add("mems", "-k", 4, "--max-occ", 3, "-o", f"{T}/out", dna, "ACGTACGTTTGCA")
    add("approx", "-d", 1, "-b", one, "ACGA")
    add("approx", "-d", 16, one, "ACGT")
    add("approx", masked, "RNELNNEEA")
    add("edit", "-d", 1, "-b", "-l", one, "ACGA")
    add("edit", "-d", 1, "-c", one, "ACGA", "ACGTT")
    add("edit", "-d", 2, "-c", "-a", "-o", f"{T}/out", dna, "ACGTACGTTTGCA")
    add("edit", masked, "RNELNNEEA")
    add("edit", "-k", 3, one, "ACGT")
    add("list", "-rsp", one)
    add("summarize", three)
    return r


SANITIZER_START = re.compile(r"^(=+\d+=+\s*ERROR|=+\s*$|.*runtime error:)")


def split_sanitizer(stderr: str):
    """(the program's own stderr, the SUMMARY lines of sanitizer reports)"""
    own, summaries, inside = [], [], False
    for line in stderr.splitlines(keepends=True):
        if not inside and SANITIZER_START.match(line):
            inside = True
            if own and own[-1] == "\n":                     # (the blank line a report starts with)
                own.pop()
        if inside:
            if line.startswith("SUMMARY: "):
                summaries.append(re.sub(r"0x[0-9a-f]+", "0x?", line.strip()))
        else:
            own.append(line)
    return "".join(own), summaries


def transcript(binary: Path, outfile: Path, legs, device: int, timeout: float) -> int:
    out, status, count = [], 0, {leg: 0 for leg in legs}
    for leg in legs:
        for row in rows():
            if leg == "device":
                if row[0] not in TAKES_DEVICE:
                    continue
                row = row + ["--device", str(device)]
            with tempfile.TemporaryDirectory() as tmp:
                argv = [a.replace(G, str(GOLDEN)).replace(T, tmp) for a in row]
                try:
                    p = subprocess.run([str(binary), *argv], capture_output=True, timeout=timeout, stdin=subprocess.DEVNULL)
                    code, so, se = p.returncode, p.stdout, p.stderr
                except subprocess.TimeoutExpired as e:
                    code, so, se = "timeout", e.stdout or b"", e.stderr or b""
                norm = lambda b: b.decode("latin-1").replace(str(GOLDEN), G).replace(tmp, T)
                own, summaries = split_sanitizer(norm(se))
                files = sorted(q for q in Path(tmp).rglob("*") if q.is_file())
                count[leg] += 1
                out.append(f"== {leg} {count[leg]}: sufr {' '.join(row)}\nexit: {code}\n")
                out.append("stdout:\n" + norm(so) + "stderr:\n" + own)
                out += [f"sanitizer: {s}\n" for s in summaries]
                out += [f"file: {q.relative_to(tmp)} {q.stat().st_size} {hashlib.sha256(q.read_bytes()).hexdigest()}\n" for q in files]
            print(f"{leg} {count[leg]}: exit {code}: sufr {' '.join(row)}", flush=True)
            if code == "timeout" or code < 0:
                out.append("== stopped: the row above died of a signal or ran out of time\n")
                status = 3
                break
        if status:
            break
    out.append("== rows: " + ", ".join(f"{leg} {n}" for leg, n in count.items()) + "\n")
    outfile.write_text("".join(out), encoding="latin-1")
    return status


def parse(path: Path):
    blocks, key = {}, None
    for line in path.read_text(encoding="latin-1").splitlines(keepends=True):
        if line.startswith("== "):
            key = line.strip()
            blocks[key] = []
        elif key is not None:
            blocks[key].append(line)
    return blocks


def compare(a: Path, b: Path) -> int:
    A, B = parse(a), parse(b)
    differ, only_reports = [], []
    for key in sorted(set(A) | set(B), key=lambda k: (list(A).index(k) if k in A else len(A), k)):
        x, y = A.get(key), B.get(key)
        if x == y:
            continue
        strip = lambda blk: [l for l in blk if not l.startswith("sanitizer: ")]
        reports = lambda blk: [l for l in blk if l.startswith("sanitizer: ")]
        if x is not None and y is not None and strip(x) == strip(y) and set(reports(y)) <= set(reports(x)):
            only_reports.append(key)
        else:
            differ.append(key)
    print(f"{len(A)} blocks in {a.name}, {len(B)} in {b.name}: {len(differ)} differ, "
          f"{len(only_reports)} differ only by sanitizer summaries that {a.name} has and {b.name} has not")
    for key in differ:
        print("DIFFERS  ", key)
    for key in only_reports:
        print("REPORT GONE", key)
    return 1 if differ else 0


def main(argv) -> int:
    if len(argv) == 3 and argv[0] == "--compare":
        return compare(Path(argv[1]), Path(argv[2]))
    if len(argv) < 2:
        print(__doc__, file=sys.stderr)
        return 2
    legs, device, timeout = ["host"], 0, 120.0
    for i in range(2, len(argv) - 1, 2):
        if argv[i] == "--legs":
            legs = argv[i + 1].split(",")
        elif argv[i] == "--device":
            device = int(argv[i + 1])
        elif argv[i] == "--timeout":
            timeout = float(argv[i + 1])
        else:
            print(__doc__, file=sys.stderr)
            return 2
    return transcript(Path(argv[0]).resolve(), Path(argv[1]), legs, device, timeout)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
