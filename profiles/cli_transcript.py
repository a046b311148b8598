#!/usr/bin/env python3
"""A transcript of the `sufr` CLI on the golden files, to compare two builds byte for byte.

    cli_transcript.py BINARY OUTFILE [--legs host,device] [--device ID] [--timeout SECONDS] [--only CMD,CMD,...]
    cli_transcript.py --compare A B

A fixed list of invocations (rows() below) runs one process each, in order, on tests/golden/expected.  OUTFILE gets, per row,
the argv, the exit status, standard output, standard error and the sha256 of every file the row wrote (-o, --occ, --unique),
with the golden directory and the row's scratch directory replaced by <GOLDEN> and <TMP>.  The `host` leg runs the rows as
listed; the `device` leg appends `--device ID` to every row whose sub-command takes it; --only keeps the rows of the named
sub-commands.  The run ends at the first row that dies of a signal or runs into its time limit (exit status 3): nothing is
started on a device after a fault.

Before the legs, setup_rows() runs once, with the same binary and recorded like rows, in a directory all rows share (<FM>):
what the `fm` rows read, the reversed FASTA of one golden file and its .sufr, and index files saved with --text, without it and
at -s 0.  `sufr create` builds on a GPU; where there is none the set-up records its refusal and the CPU oracle writes that
.sufr (recorded too).

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
G, T, F = "<GOLDEN>", "<TMP>", "<FM>"
TAKES_DEVICE = {"count", "co", "locate", "lo", "extract", "ex", "match", "ma", "mems", "me", "approx", "ap", "edit", "ed",
                "kmers", "km", "repeats", "rp", "shared", "lz", "bwt", "fm"}
FM_SOURCE = "2ns.sufr"                  # 18 positions in two sequences, --dna --allow-ambiguity --ignore-softmask
FM_READS = ">r1\nACGTN\n>r2\nNNAC\n>r3\nTTT\n"


def setup_rows():
    ns = f"{G}/{FM_SOURCE}"
    return [["fm", ns, "--write-reverse", f"{F}/rev.fa"],
            ["create", "--dna", "--allow-ambiguity", "--ignore-softmask", "-o", f"{F}/rev.sufr", f"{F}/rev.fa"],
            ["fm", ns, "--save", f"{F}/text.fm", "--text", "-s", "4"],
            ["fm", ns, "--save", f"{F}/plain.fm", "-s", "4"],
            ["fm", ns, "--save", f"{F}/bare.fm", "-s", "0"],
            ["fm", f"{F}/rev.sufr", "--save", f"{F}/rev.fm", "-s", "0"]]


def oracle_create(fasta: Path, out: Path):
    """the .sufr of `fasta` with the flags of FM_SOURCE, by the CPU oracle"""
    sys.path.insert(0, str(ROOT / "tests"))
    from oracle_helper import Oracle
    Oracle().create(fasta, out, is_dna=True, allow_ambiguity=True, ignore_softmask=True)
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
    # -- bwt -----------------------------------------------------------------------------------------------------------
    add("bwt", one)
    add("bwt", "--runs", three)
    add("bwt", "--runs", "--min-len", 2, "-o", f"{T}/out", uni)
    add("bwt", "--bwt", f"{T}/bwt", "--lf", f"{T}/lf", "-t", 2, dna)
    add("bwt", masked)
    add("bwt", f"{G}/no-such-file.sufr")
    add("bwt", "-o", f"{T}/no-such-dir/out", one)
    add("bwt", "--bwt", f"{T}/no-such-dir/bwt", one)
    # -- fm: count, locate, --mismatches on an index built from the file -------------------------------------------------
    ns, amb, missing, nodir = f"{G}/{FM_SOURCE}", f"{G}/long_dna_sequence_allow_ambiguity.sufr", f"{G}/no-such-file.sufr", f"{T}/no-such-dir/out"
    add("fm", ns, "AC", "GT", "N", "TTT")
    add("fm", "--locate", ns, "AC", "GT", "N", "TTT")
    add("fm", "--locate", "-a", ns, "AC", "N")
    add("fm", "--locate", "-s", 0, ns, "AC", "N")                                    # built at sample 1
    add("fm", "--locate", "--sample", 3, "--max-hits", 2, ns, "N", "ACGT", "")
    add("fm", "-s", 0, ns, "AC")
    add("fm", "-o", f"{T}/out", "-q", f"{F}/reads.fa", ns, "AC")
    add("fm", "--locate", "-o", f"{T}/out", "-t", 2, uni, "RNELNNEEA", "MSF", "ZZZZ")
    add("fm", "--locate", "--max-hits", 3, "-a", amb, "ACGTAC", "GATTACA")
    add("fm", "-d", 1, ns, "ACGA", "NNNT", "TTTTTT")
    add("fm", "--mismatches", 1, "-b", "-a", "-q", f"{F}/reads.fa", ns)
    add("fm", "-d", 0, "-s", 5, "-o", f"{T}/out", amb, "ACGTACGT")
    add("fm", "-d", 2, "-t", 2, uni, "RNELNNEEA")                                    # more records than the first capacity
    add("fm", "-d", 4, ns, "ACGT")
    add("fm", "-d", 1, "-s", 0, ns, "ACGT")
    add("fm", "-d", 4, missing, "ACGT")
    add("fm", "-d", 1, "-s", 0, missing, "ACGT")
    add("fm", "-d", 1, "-o", nodir, missing, "ACGT")
    add("fm", "-d", 1, "-o", nodir, ns, "ACGT")
    add("fm", "-d", 1, one, "AC")
    add("fm", "-d", 1, masked, "RNEL")
    add("fm", one, "AC")
    add("fm", "--locate", one, "AC")
    add("fm", masked, "RNEL")
    add("fm", missing, "AC")
    add("fm", "-o", nodir, ns, "AC")
    add("fm", "-o", nodir, missing, "AC")
    add("fm", "-q", f"{T}/no-such-reads.fa", ns)
    add("fm", ns)
    add("fm")
    add("fm", ns, "AC", "-s")
    add("fm", ns, "--bogus", "AC")
    # -- fm --index / --save / --text / --extract ------------------------------------------------------------------------------
    text, plain, bare = f"{F}/text.fm", f"{F}/plain.fm", f"{F}/bare.fm"
    add("fm", "--index", text, "AC", "N", "TTT")
    add("fm", "--index", text, "--locate", "AC", "N", "TTT")
    add("fm", "--index", plain, "--locate", "-a", "--max-hits", 1, "N", "-q", f"{F}/reads.fa")
    add("fm", "--index", text, "-d", 1, "-b", "ACGA", "NNNT")
    add("fm", "--index", text, "--extract", "AC", "TTT")
    add("fm", "--index", text, "--extract", "--prefix-len", 1, "--suffix-len", 3, "-o", f"{T}/out", "CG", "N")
    add("fm", "--index", text, "--extract", "--max-hits", 1, "N")                    # --extract takes every hit
    add("fm", "--index", plain, "--extract", "AC")
    add("fm", "--index", bare, "AC", "N")
    add("fm", "--index", bare, "--locate", "AC")
    add("fm", "--index", bare, "-d", 1, "ACGT")
    add("fm", "--index", bare, "--extract", "AC")
    add("fm", "--index", text, "-d", 4, "ACGT")
    add("fm", "--index", text, "-d", 1, "-s", 0, "ACGT")
    add("fm", "--index", f"{F}/no-such-file.fm", "AC")
    add("fm", "--index", ns, "AC")                                                   # not an index file
    add("fm", "--index", text, "-o", nodir, "AC")
    add("fm", "--index", f"{F}/no-such-file.fm", "-o", nodir, "AC")
    add("fm", "--index", text)
    add("fm", ns, "--save", f"{T}/x.fm")                                             # --save alone
    add("fm", ns, "--save", f"{T}/x.fm", "--text", "-s", 2, "--locate", "AC")
    add("fm", ns, "--save", f"{T}/x.fm", "-s", 0, "AC")
    add("fm", ns, "--save", f"{T}/x.fm", "-s", 0, "--locate", "AC")
    add("fm", ns, "--save", f"{T}/no-such-dir/x.fm", "AC")
    add("fm", ns, "--text", "AC")
    add("fm", ns, "--text", "-s", 0, "AC")
    add("fm", ns, "--text", "--locate", "AC", "TTT")
    add("fm", ns, "--extract", "AC", "TTT")
    add("fm", ns, "--extract", "-d", 1, "ACGA")
    add("fm", uni, "--extract", "--prefix-len", 2, "--suffix-len", 5, "-s", 7, "-t", 2, "RNELNNEEA")
    add("fm", one, "--save", f"{T}/x.fm")
    add("fm", masked, "--extract", "RNEL")
    add("fm", missing, "--text", "AC")
    add("fm", missing, "--text", "-o", nodir, "AC")
    add("fm", missing, "--text", "-d", 4, "AC")
    # -- fm --write-reverse / --smems --reverse ---------------------------------------------------------------------------------
    rev, rev_fm = f"{F}/rev.sufr", f"{F}/rev.fm"
    add("fm", ns, "--smems", "--reverse", rev, "-k", 2, "ACGTN", "NNAC", "TTT")
    add("fm", ns, "--smems", "--reverse", rev_fm, "-k", 2, "-a", "--max-hits", 1, "ACGTN", "NNNN")
    add("fm", ns, "--smems", "--reverse", rev, "--min-len", 1, "--max-hits", 2, "-s", 3, "NNNNACGT")
    add("fm", "--index", plain, "--smems", "--reverse", rev_fm, "-k", 3, "-o", f"{T}/out", "-q", f"{F}/reads.fa")
    add("fm", "--index", text, "--smems", "--reverse", rev, "-k", 2, "-t", 2, "ACGTN")
    add("fm", ns, "--smems", "--reverse", rev, "ACGTNNNN")                           # -k 20: no record
    add("fm", uni, "--smems", "--reverse", uni, "-k", 5, "RNELNNEEA")                # passes the pair check of the host: not refused there
    add("fm", ns, "--write-reverse", f"{T}/w.fa", "--smems", "--reverse", rev, "-k", 2, "ACGTN")
    add("fm", ns, "--write-reverse", f"{T}/w.fa")
    add("fm", uni, "--write-reverse", f"{T}/w.fa", "-o", f"{T}/out")
    add("fm", ns, "--write-reverse", f"{T}/no-such-dir/w.fa", "--smems", "--reverse", rev, "-k", 2, "ACGTN")
    add("fm", "--index", text, "--write-reverse", f"{T}/w.fa")
    add("fm", ns, "--reverse", rev, "ACGT")
    add("fm", ns, "--smems", "ACGT")
    add("fm", ns, "--smems", "--reverse", f"{G}/abba.sufr", "-k", 2, "ACGT")
    add("fm", ns, "--smems", "--reverse", rev, "-s", 0, "ACGT")
    add("fm", "--index", bare, "--smems", "--reverse", rev_fm, "-k", 2, "ACGT")
    add("fm", ns, "--smems", "--reverse", rev, "-k", 0, "ACGT")
    add("fm", ns, "--smems", "--reverse", f"{F}/no-such-file", "ACGT")
    add("fm", one, "--smems", "--reverse", rev, "-k", 2, "ACGT")
    add("fm", masked, "--smems", "--reverse", rev, "-k", 2, "ACGT")
    add("fm", ns, "--smems", "--reverse", masked, "-k", 2, "ACGT")
    add("fm", missing, "--smems", "--reverse", rev, "-k", 2, "ACGT")
    add("fm", ns, "--smems", "--reverse", rev, "-o", nodir, "ACGT")
    add("fm", ns, "--smems", "--reverse", rev, "-q", f"{T}/no-such-reads.fa")
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


def file_lines(folder: str):
    files = sorted(q for q in Path(folder).rglob("*") if q.is_file())
    return [f"file: {q.relative_to(folder)} {q.stat().st_size} {hashlib.sha256(q.read_bytes()).hexdigest()}\n" for q in files]


def run_row(binary: Path, label: str, row, shared: str, timeout: float, out, wrote_in=None):
    """One process: its block goes to `out` with the files of its own scratch directory (or of `wrote_in`).  Returns the exit
    status, "timeout" for a row that ran out of time."""
    with tempfile.TemporaryDirectory() as tmp:
        argv = [a.replace(G, str(GOLDEN)).replace(T, tmp).replace(F, shared) for a in row]
        try:
            p = subprocess.run([str(binary), *argv], capture_output=True, timeout=timeout, stdin=subprocess.DEVNULL)
            code, so, se = p.returncode, p.stdout, p.stderr
        except subprocess.TimeoutExpired as e:
            code, so, se = "timeout", e.stdout or b"", e.stderr or b""
        norm = lambda b: b.decode("latin-1").replace(str(GOLDEN), G).replace(tmp, T).replace(shared, F)
        own, summaries = split_sanitizer(norm(se))
        out.append(f"== {label}: sufr {' '.join(row)}\nexit: {code}\n")
        out.append("stdout:\n" + norm(so) + "stderr:\n" + own)
        out += [f"sanitizer: {s}\n" for s in summaries]
        out += file_lines(wrote_in or tmp)
    print(f"{label}: exit {code}: sufr {' '.join(row)}", flush=True)
    return code


def transcript(binary: Path, outfile: Path, legs, device: int, timeout: float, only=None) -> int:
    out, status, count = [], 0, {leg: 0 for leg in legs}
    died = lambda code: code == "timeout" or code < 0
    with tempfile.TemporaryDirectory() as shared:
        Path(shared, "reads.fa").write_text(FM_READS)
        for n, row in enumerate(setup_rows(), 1):
            if died(run_row(binary, f"setup {n}", row, shared, timeout, out, wrote_in=shared)):
                status = 3
                break
            if row[0] == "create" and not Path(shared, "rev.sufr").exists():
                oracle_create(Path(shared, "rev.fa"), Path(shared, "rev.sufr"))
                out += [f"== setup {n}, by the oracle\n"] + file_lines(shared)
        for leg in legs:
            for row in [] if status else rows():
                if only and row[0] not in only:
                    continue
                if leg == "device":
                    if row[0] not in TAKES_DEVICE:
                        continue
                    row = row + ["--device", str(device)]
                count[leg] += 1
                if died(run_row(binary, f"{leg} {count[leg]}", row, shared, timeout, out)):
                    status = 3
                    break
    if status:
        out.append("== stopped: the row above died of a signal or ran out of time\n")
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
    legs, device, timeout, only = ["host"], 0, 120.0, None
    for i in range(2, len(argv) - 1, 2):
        if argv[i] == "--legs":
            legs = argv[i + 1].split(",")
        elif argv[i] == "--device":
            device = int(argv[i + 1])
        elif argv[i] == "--timeout":
            timeout = float(argv[i + 1])
        elif argv[i] == "--only":
            only = set(argv[i + 1].split(","))
        else:
            print(__doc__, file=sys.stderr)
            return 2
    return transcript(Path(argv[0]).resolve(), Path(argv[1]), legs, device, timeout, only)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
