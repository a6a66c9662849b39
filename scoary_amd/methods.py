"""Host-side mirror of the reference's interface for the association path.

Same entry points, argument meaning and result shapes as scoary/methods.py of
AdmiralenOla/Scoary v1.6.16 -- but array-based inside, with every count,
Fisher test and permutation evaluated by the HIP library (scoary_amd.engine):

  Csv_to_dic_Roary   scoary/methods.py:335-508   gene presence/absence reader
  Csv_to_dic         scoary/methods.py:546-614   traits reader
  Perform_statistics scoary/methods.py:930-982   one (gene, trait) 2x2 table
  Setup_results      scoary/methods.py:757-928   counts + Fisher + B/BH per trait
  Permute            scoary/methods.py:1314-1369 empirical p (Fisher statistic,
                                                 SURVEY D1 / DESIGN.md)
  StoreResults / StoreTraitResult  :987-1197     per-trait results CSV
  ScoaryArgumentParser / main      :1551-1744, :49-330   the CLI

There is no CPU fallback: without the GPU library these functions raise.
"""
import argparse
import csv
import logging
import os
import re
import sys
import time as _time
from collections import namedtuple
from collections.abc import Mapping

import numpy as np

from . import SCOARY_COMPAT_VERSION, __version__
from .engine import AssociationEngine, pack_bits_rows

log = logging.getLogger("scoary_amd")
log.setLevel(logging.DEBUG)

ABSENT_CELLS = ("", "0", "-")                     # methods.py:476
MISSING_TRAIT = ("NA", "-", ".", " ", "")         # methods.py:592
ALLOWED_TRAIT = ("0", "1") + MISSING_TRAIT        # methods.py:576
ROARY_HEAD = ["Gene", "Non-unique Gene name", "Annotation"]
ROARY_COLS = set(ROARY_HEAD + [
    "No. isolates", "No. sequences", "Avg sequences per isolate", "Genome Fragment",
    "Order within Fragment", "Accessory Fragment", "Accessory Order with Fragment", "QC",
    "Min group size nuc", "Max group size nuc", "Avg group size nuc",
    "Order within fragment", "Genome fragment", "Accessory fragment"])

DEFAULT_SEED = 0x5C0A27


# ---------------------------------------------------------------------------
# Input containers
# ---------------------------------------------------------------------------
class GeneTable(Mapping):
    """The reference's ``genedic`` (gene id -> {strain: 0/1, "Non-unique Gene
    name", "Annotation", "<col>_name"}) held as arrays: ordered ids, metadata
    columns and bit-packed presence rows (rows64, spec S1).  Behaves as a
    read-only mapping with the reference's shape, so code written against
    ``genedic[gene][strain]`` keeps working."""

    def __init__(self, ids, nugn, annotation, strains, rows64, extra=None):
        self.ids = list(ids)
        self.nugn = list(nugn)
        self.annotation = list(annotation)
        self.strains = list(strains)
        self.rows64 = np.ascontiguousarray(rows64, dtype=np.uint64)
        self.extra = extra or {}                 # "<col>_name" -> list per gene
        self._index = {g: i for i, g in enumerate(self.ids)}
        self._device = None                      # (engine, GeneMatrix) cache

    @classmethod
    def from_genedic(cls, genedic, strains=None):
        """Pack a plain reference-style dict of dicts."""
        ids = list(genedic.keys())
        meta = ("Non-unique Gene name", "Annotation")
        if strains is None:
            first = genedic[ids[0]] if ids else {}
            strains = [k for k in first if k not in meta and not str(k).endswith("_name")]
        dense = np.zeros((len(ids), len(strains)), dtype=np.uint8)
        for i, g in enumerate(ids):
            row = genedic[g]
            dense[i] = [1 if row[s] else 0 for s in strains]
        extra_keys = [k for k in (genedic[ids[0]] if ids else {}) if str(k).endswith("_name")]
        extra = {k: [genedic[g].get(k, "") for g in ids] for k in extra_keys}
        return cls(ids, [genedic[g].get(meta[0], "") for g in ids],
                   [genedic[g].get(meta[1], "") for g in ids], strains,
                   pack_bits_rows(dense), extra)

    # Mapping interface --------------------------------------------------
    def __len__(self):
        return len(self.ids)

    def __iter__(self):
        return iter(self.ids)

    def __getitem__(self, gene):
        i = self._index[gene]
        bits = np.unpackbits(self.rows64[i].view(np.uint8), bitorder="little")
        row = {"Non-unique Gene name": self.nugn[i], "Annotation": self.annotation[i]}
        for j, s in enumerate(self.strains):
            row[s] = int(bits[j])
        for k, col in self.extra.items():
            row[k] = col[i]
        return row

    def index(self, gene):
        return self._index[gene]

    def dense(self):
        """(G, N) uint8 presence matrix."""
        N = len(self.strains)
        by = self.rows64.view(np.uint8).reshape(len(self.ids), -1)
        return np.unpackbits(by, axis=1, bitorder="little")[:, :N]

    def on_device(self, engine):
        if self._device is None or self._device[0] is not engine:
            self._device = (engine, engine.tile_rows(self.rows64, len(self.strains)))
        return self._device[1]


def _trait_arrays(traitsdic, strains):
    """traitsdic (trait -> {strain: "0"/"1"}, missing isolates absent) ->
    names, (T, N) uint8 with 2 = missing.  A strain named in a trait but not in
    the gene table is the reference's fatal KeyError path (methods.py:974-980)."""
    names = list(traitsdic.keys())
    col = {s: j for j, s in enumerate(strains)}
    arr = np.full((len(names), len(strains)), 2, dtype=np.uint8)
    for t, name in enumerate(names):
        for s, v in traitsdic[name].items():
            if s not in col:
                log.critical("CRITICAL: Could not find %s in the genes file." % str(s))
                sys.exit("Make sure strains are named the same in your traits file as in "
                         "your gene presence/absence file")
            if v in ("0", "1", 0, 1):
                arr[t, col[s]] = int(v)
            elif v in MISSING_TRAIT or v == "NA":
                arr[t, col[s]] = 2
            else:
                sys.exit("There was a problem with comparing your traits and gene "
                         "presence/absence files: unexpected trait value %r" % (v,))
    return names, arr


class TraitResults(Mapping):
    """``Results[trait]``: gene -> row dict, array-backed (one numpy column per
    field, rows materialised on access).  Keys are the testable genes in the
    reference's insertion order."""

    FIELDS = ("tpgp", "tngp", "tpgn", "tngn", "sens", "spes", "OR", "p_v", "B_p", "BH_p")

    def __init__(self, genes, nugn, annotation, cols, number_of_tests, members=None, table=None,
                 rows_idx=None):
        """Either explicit name lists (``genes`` / ``nugn`` / ``annotation``: the --collapse units,
        plain reference dicts) or -- the common case -- ``table`` + ``rows_idx``: row i is gene
        ``rows_idx[i]`` of the GeneTable and its names are looked up when asked for.  A result set
        of G genes x T traits then costs T index arrays, not G x T Python strings; only the rows
        that are written (or read through the mapping interface) are ever materialised."""
        self._table, self._rows_idx = table, rows_idx
        self._genes = None if table is not None else list(genes)
        self._nugn = None if table is not None else list(nugn)
        self._annotation = None if table is not None else list(annotation)
        self.cols = cols                         # field -> ndarray
        self.number_of_tests = number_of_tests
        self.members = members                   # collapse: row -> list of source gene ids
        self._index_cache = None
        self.p_order = None                      # stable argsort of cols["p_v"], if already known

    # names of one row: O(1), nothing materialised
    def gene_at(self, i):
        return self._genes[i] if self._genes is not None else self._table.ids[self._rows_idx[i]]

    def nugn_at(self, i):
        return self._nugn[i] if self._nugn is not None else self._table.nugn[self._rows_idx[i]]

    def annotation_at(self, i):
        return self._annotation[i] if self._annotation is not None \
            else self._table.annotation[self._rows_idx[i]]

    def source_index(self, i):
        """Row of the GeneTable behind result row i (the last member of a --collapse unit)."""
        if self._rows_idx is not None:
            return int(self._rows_idx[i])
        return None

    # whole name lists (the reference's dict view): built on first use
    @property
    def genes(self):
        if self._genes is None:
            ids = self._table.ids
            self._genes = [ids[i] for i in self._rows_idx]
        return self._genes

    @property
    def nugn(self):
        if self._nugn is None:
            v = self._table.nugn
            self._nugn = [v[i] for i in self._rows_idx]
        return self._nugn

    @property
    def annotation(self):
        if self._annotation is None:
            v = self._table.annotation
            self._annotation = [v[i] for i in self._rows_idx]
        return self._annotation

    @property
    def _index(self):
        if self._index_cache is None:
            self._index_cache = {g: i for i, g in enumerate(self.genes)}
        return self._index_cache

    def __len__(self):
        return len(self._rows_idx) if self._genes is None else len(self._genes)

    def __iter__(self):
        return iter(self.genes)

    def __getitem__(self, gene):
        i = self._index[gene]
        row = {"NUGN": self.nugn_at(i), "Annotation": self.annotation_at(i)}
        for k, col in self.cols.items():
            v = col[i]
            row[k] = int(v) if k in ("tpgp", "tngp", "tpgn", "tngn") else \
                (float(v) if k in ("sens", "spes") else v)
        return row

    def column(self, name):
        return self.cols[name]


class GeneTraitCombinations(Mapping):
    """``Gene_trait_combinations[trait]``: gene -> {strain: "AB"|"Ab"|"aB"|"ab"}
    over the trait's valid isolates (methods.py:953-965), computed lazily --
    only the tree stage of the reference consumes it."""

    def __init__(self, table, genes, members, trait_row, trait_index=0):
        """``genes``: a list of names or the trait's TraitResults (names looked up on demand)."""
        self.table, self._names, self.members, self.trait_row = table, genes, members, trait_row
        self.trait_index = trait_index           # enters the permutation counters (spec S4)
        self._index_cache = None

    @property
    def genes(self):
        return self._names.genes if isinstance(self._names, TraitResults) else self._names

    @property
    def _index(self):
        if self._index_cache is None:
            self._index_cache = {g: i for i, g in enumerate(self.genes)}
        return self._index_cache

    def __len__(self):
        return len(self._names)

    def __iter__(self):
        return iter(self.genes)

    def __getitem__(self, gene):
        i = self._index[gene]
        src = self.members[i][-1] if self.members is not None else gene
        gi = self.table.index(src)
        bits = np.unpackbits(self.table.rows64[gi].view(np.uint8), bitorder="little")
        out = {}
        for j, s in enumerate(self.table.strains):
            t = self.trait_row[j]
            if t == 2:
                continue
            out[s] = ("A" if bits[j] else "a") + ("B" if t == 1 else "b")
        return out


# ---------------------------------------------------------------------------
# Stage clock: seconds per named stage of a command-line run ("Stage detail" log line)
# ---------------------------------------------------------------------------
class _Stages:
    def __init__(self):
        self.seconds = {}

    def reset(self):
        self.seconds = {}

    def __call__(self, name):
        return _StageTimer(self, name)


class _StageTimer:
    def __init__(self, owner, name):
        self.owner, self.name = owner, name

    def __enter__(self):
        self.t0 = _time.perf_counter()
        return self

    def __exit__(self, *exc):
        self.owner.seconds[self.name] = self.owner.seconds.get(self.name, 0.0) + _time.perf_counter() - self.t0
        return False


_stage = _Stages()


# ---------------------------------------------------------------------------
# Engine singleton
# ---------------------------------------------------------------------------
_ENGINE = None


def _preload_scipy():
    """Default (pairwise) mode may ask SciPy for a few binomial tails (tree.binom_two_sided_many: the central pairs of
    genes with 79 or more contrasting pairs); importing scipy.stats takes 0.3-0.5 s, so it starts here, on a helper
    thread under the association stage, instead of in the middle of the first trait's pairwise stage."""
    import threading

    def load():
        try:
            import scipy.stats  # noqa: F401
        except ImportError:
            pass
    threading.Thread(target=load, name="scoary-scipy-preload", daemon=True).start()


def get_engine():
    global _ENGINE
    if _ENGINE is None:
        eng = AssociationEngine()
        try:
            _warm_up(eng)
        except Exception as e:      # only an optimisation: a tiny list budget, a failed LDS opt-in or an
            log.debug("engine warm-up skipped: %s: %s" % (type(e).__name__, e))   # OOM must not cost the run
        _ENGINE = eng
    return _ENGINE


def _warm_up(eng):
    """One tiny pass through the path when the engine is created: the first launch of the
    library loads its code object, the first copies set up torch's allocator and staging
    buffers -- tens of milliseconds that belong to process start-up, not to the association
    stage of the first (and usually only) data set."""
    import torch
    g = eng.pack_dense(np.array([[1, 0, 1, 0], [0, 1, 1, 0]], dtype=np.uint8))
    lab = pack_bits_rows(np.array([[1, 1, 0, 0]], dtype=np.uint8))
    val = pack_bits_rows(np.ones((1, 4), dtype=np.uint8))
    trv, mkv = eng.vecrows(lab, 4), eng.vecrows(val, 4)
    eng.build_lists(g)
    res = eng.associate(g, trv, mkv, permutations=32, seed=1)
    eng.pack_records(res).cpu()
    torch.cuda.synchronize(eng.device)


# ---------------------------------------------------------------------------
# Readers
# ---------------------------------------------------------------------------
def _is_roary_file(path, delimiter):
    """Does the table's header start with Roary's three columns (methods.py:373-376)?"""
    try:
        with open(path, "r") as f:
            return next(csv.reader(f, skipinitialspace=True, delimiter=delimiter))[0:3] == ROARY_HEAD
    except (OSError, StopIteration, UnicodeError):
        return True


def Csv_to_dic_Roary(genefile, delimiter, grabcols, startcol=14, allowed_isolates=None,
                     writereducedset=False, time="", outdir="./"):
    """Read a Roary-style gene presence/absence table (methods.py:335-508).

    Returns the reference's dict: "Roarydic" (a GeneTable), "Zero_ones_matrix"
    (strain-major 0/1 lists of the variable genes, for tree building),
    "Strains", "Extracols", "Firstcolnames".  Plain files are tokenised by the
    native streaming reader (scoary_amd/csrc/scoary_io.cpp, same csv dialect);
    other handles, or --include_input_columns reaching into strain columns, go
    through Python's csv module."""
    opened = None
    if writereducedset:
        # under torchrun only rank 0 writes the reduced table; the other ranks wait for it
        # (all ranks writing the same path with mode "w" raced each other's reads)
        from . import dist as _dist
        world, rank = _dist.world_rank()
        name = _reduced_name(outdir, time)
        if world > 1:
            # every rank built `time` from its own clock: ranks that straddle a minute would
            # look for a file rank 0 never wrote -- rank 0's name is the name
            name = _dist.all_gather_objects(name)[0]
        if rank == 0:
            ReduceSet(genefile, delimiter, grabcols, startcol, allowed_isolates, time, outdir)
        if world > 1:
            _dist.barrier()
        opened = open(name, "r", newline=None)
        genefile = opened
    from . import io_native
    path = getattr(genefile, "name", None)
    native = (io_native.available() and isinstance(path, str) and os.path.isfile(path)
              and len(delimiter) == 1 and delimiter not in ' "\r\n'
              and os.environ.get("SCOARY_PY_CSV") != "1"
              and startcol >= 3          # a -s inside the identifier cells (or negative: Python's slices): the csv path
              and grabcols != [-999] and all(0 <= c < startcol for c in grabcols))
    rows_iter = None
    if native:
        try:
            def wanted(hdr):     # identifier, name and annotation columns + the grabbed ones
                try:
                    first = [hdr.index(h) for h in ROARY_HEAD] if hdr[0:3] == ROARY_HEAD else [0, 1, 2]
                except ValueError:
                    first = [0, 1, 2]
                return first + list(grabcols)
            header, meta_rows, bits, kept_native = _read_gpa_ranks(
                io_native, path, delimiter, startcol, allowed_isolates, wanted)
        except io_native.GpaError as e:
            if "startcol" in str(e):
                sys.exit("The startcol (-s) you have specified does not seem to correspond to "
                         "any column in your gene presence/absence file.")
            # the reference's two messages (methods.py:447-462): a data row too short to hold its
            # identifier cells ends a Roary table with the first, a plain table with the second;
            # the reader's own description of the row goes to the log, not into the message
            log.debug("gene presence absence reader: %s" % e)
            short = re.search(r"row \d+ has (\d+) cells", str(e))
            if short and int(short.group(1)) < 3 and not _is_roary_file(path, delimiter):
                sys.exit("CRITICAL: Could not properly assign column. Please report this bug.")
            sys.exit("CRITICAL: Could not read gene presence absence file. Verify that this "
                     "file is a proper Roary file using the specified delimiter (default is "
                     "',').")
    else:
        reader = csv.reader(genefile, skipinitialspace=True, delimiter=delimiter)
        header = next(reader)
        rows_iter = reader
    if grabcols == [-999]:
        grabcols = list(range(3, len(header)))
    if startcol >= len(header):
        sys.exit("The startcol (-s) you have specified does not seem to correspond to any "
                 "column in your gene presence/absence file.")
    strains = header[startcol:]
    extracols = [header[c] for c in grabcols]
    roary = header[0:3] == ROARY_HEAD

    # -s sanity hints (methods.py:382-414): same diagnostics, same conditions
    if roary and strains[0] in ROARY_COLS:
        guess = next((startcol + c for c, s in enumerate(strains) if s not in ROARY_COLS), None)
        log.error("ERROR: Make sure you have set the -s parameter correctly. You are running "
                  "with -s %s. This correponds to the column %s. If this is not an isolate, "
                  "Scoary might crash or produce strange results. Scoary thinks you should have "
                  "run with -s %s instead" % (startcol + 1, strains[0],
                                              (guess + 1) if guess is not None else "?"))
    if roary:
        suspicious = []
        for name in reversed(header[:startcol]):
            if name not in ROARY_COLS:
                suspicious.append(name)
            else:
                if suspicious:
                    log.error("ERROR: Make sure you have set the -s parameter correctly. You "
                              "are running with -s %s. Scoary thinks you should have used %s. "
                              "This excludes the following, which Scoary thinks are isolates: %s"
                              % (startcol + 1, startcol - len(suspicious) + 1,
                                 ", ".join(suspicious)))
                break

    keep = [c for c, s in enumerate(strains)
            if allowed_isolates is None or s in allowed_isolates]
    kept_strains = [strains[c] for c in keep]
    if roary:
        try:
            genecol, nugcol, anncol = (header.index(h) for h in ROARY_HEAD)
        except ValueError:
            genecol, nugcol, anncol = 0, 1, 2
        firstcolnames = list(ROARY_HEAD)
    else:
        genecol, nugcol, anncol = 0, 1, 2
        firstcolnames = header[0:3]

    # a repeated identifier replaces the earlier row but keeps its position
    # (dict overwrite in the reference)
    index, ids, nugn, ann, source = {}, [], [], [], []
    extra = {header[c] + "_name": [] for c in grabcols}
    dense_rows = []
    all_rows = []        # presence of every FILE row (the tree stage uses these, see the return)

    def take(q, r, present):
        try:
            ident = q[genecol] if roary else "_|_".join((q[genecol], q[nugcol], q[anncol]))
            meta = (q[nugcol], q[anncol])
            grabbed = [q[c] for c in grabcols]
        except IndexError:
            if not roary:
                sys.exit("CRITICAL: Could not properly assign column. Please report this bug.")
            sys.exit("CRITICAL: Could not read gene presence absence file. Verify that this "
                     "file is a proper Roary file using the specified delimiter (default is ',').")
        if ident in index:
            i = index[ident]
            nugn[i], ann[i], source[i] = meta[0], meta[1], r
            if present is not None:
                dense_rows[i] = present
            for c, v in zip(grabcols, grabbed):
                extra[header[c] + "_name"][i] = v
        else:
            index[ident] = len(ids)
            ids.append(ident)
            nugn.append(meta[0])
            ann.append(meta[1])
            source.append(r)
            if present is not None:
                dense_rows.append(present)
            for c, v in zip(grabcols, grabbed):
                extra[header[c] + "_name"].append(v)

    if native:
        if startcol > max(genecol, nugcol, anncol, *grabcols, 2):
            # the native reader's rows all have startcol cells: the dict semantics of the reference
            # (a repeated identifier keeps its first position and takes the last row's content)
            # are those of dict(zip(...)) -- no per-row Python function
            idents = [q[genecol] for q in meta_rows] if roary else \
                ["_|_".join((q[genecol], q[nugcol], q[anncol])) for q in meta_rows]
            last = dict(zip(idents, range(len(idents))))
            ids, source = list(last.keys()), list(last.values())
            nugn = [meta_rows[r][nugcol] for r in source]
            ann = [meta_rows[r][anncol] for r in source]
            for c in grabcols:
                extra[header[c] + "_name"] = [meta_rows[r][c] for r in source]
        else:
            for r, q in enumerate(meta_rows):
                take(q, r, None)
        rows64 = bits[np.array(source, dtype=np.int64)] if ids else bits[:0]
        table = GeneTable(ids, nugn, ann, kept_strains, rows64, extra)
        file_rows64 = np.ascontiguousarray(bits, dtype=np.uint64)     # EVERY file row, see below
    else:
        for r, q in enumerate(rows_iter):
            try:
                present = [q[startcol + c] not in ABSENT_CELLS for c in keep]
            except IndexError:
                sys.exit("CRITICAL: Could not read gene presence absence file. Verify that "
                         "this file is a proper Roary file using the specified delimiter "
                         "(default is ',').")
            take(q, r, present)
            all_rows.append(present)
        dense = np.array(dense_rows, dtype=np.uint8).reshape(len(ids), len(keep))
        # A -s inside the identifier cells makes "Non-unique Gene name" / "Annotation" isolate columns, and in the
        # reference's dictionary the isolate's 0 / 1 then REPLACES the text stored under that key (:449-481): the
        # result files print it.  Same here (the last column of that name wins, as in a dict).
        for key, texts in (("Non-unique Gene name", nugn), ("Annotation", ann)):
            if key in kept_strains:
                c = len(kept_strains) - 1 - kept_strains[::-1].index(key)
                texts[:] = [str(int(v)) for v in dense[:, c]]
        table = GeneTable(ids, nugn, ann, kept_strains, pack_bits_rows(dense), extra)
        file_rows64 = pack_bits_rows(np.array(all_rows, dtype=np.uint8).reshape(len(all_rows), len(keep)))
    if opened is not None:
        opened.close()
    # Zero_ones_matrix comes from every row of the FILE, not from the de-duplicated table: the
    # reference appends each (variable) row as it reads it and only the dict entry of a
    # repeated identifier is overwritten (scoary/methods.py:445-497), so repeated identifiers
    # (VCF multi-allelic sites in non-Roary files) count once per row in the Hamming distances.
    return {"Roarydic": table, "Zero_ones_matrix": _LazyZeroOnes(file_rows64, len(kept_strains)),
            "Strains": kept_strains, "Extracols": extracols, "Firstcolnames": firstcolnames}


class _LazyZeroOnes:
    """``Zero_ones_matrix`` (methods.py:493-502): strain-major 0/1 lists of the
    variable genes.  Only the tree builder wants it, so the list-of-lists is
    built on first use."""

    def __init__(self, rows64, nstrains):
        self._rows64, self._n, self._lists = rows64, nstrains, None

    def file_rows(self):
        """(file rows, N) uint8 presence of every row of the gene file (what the
        reference's zero_ones_line loop sees, before the all-0 / all-1 filter)."""
        rows, words = self._rows64.shape     # explicit width: a table without data rows has size 0
        by = np.ascontiguousarray(self._rows64).view(np.uint8).reshape(rows, words * 8)
        return np.unpackbits(by, axis=1, bitorder="little")[:, :self._n]

    def _get(self):
        if self._lists is None:
            d = self.file_rows()
            tot = d.sum(axis=1) if d.size else np.zeros(0)
            var = (tot > 0) & (tot < d.shape[1])
            # no variable row: the reference transposes an empty list, zip(*[]) == [] (:499)
            self._lists = d[var].T.tolist() if d.shape[1] and var.any() else []
        return self._lists

    def __iter__(self):
        return iter(self._get())

    def __len__(self):
        return len(self._get())

    def __getitem__(self, k):
        return self._get()[k]


def _read_gpa_ranks(io_native, path, delimiter, startcol, allowed_isolates, wanted):
    """The native reader, shared between the ranks of a torchrun launch: every rank parses
    one byte range of the body (cut at line ends) and the bit rows / text columns are put
    back together with one all-gather each, instead of every rank tokenising the whole file
    (the reference's workers all receive the one parsed dict, scoary/methods.py:1083-1097;
    here the file is the thing that is big).  A boundary inside a quoted multi-line cell, or
    SCOARY_SHARDED_READ=0, makes every rank read the whole file."""
    from . import dist as _dist
    world, rank = _dist.world_rank()
    if world > 1 and os.environ.get("SCOARY_SHARDED_READ", "1") != "0":
        part, status = None, "ok"
        try:
            part = io_native.read_gpa(path, delimiter, startcol, allowed_isolates,
                                      need_cols=wanted, part=(rank, world))
        except io_native.GpaPartBoundary:
            status = "boundary"
        except io_native.GpaError as e:
            status = "error:" + str(e)
        except Exception as e:   # OSError, MemoryError, ctypes failure: still reach the gather,
            status = "fatal:%s: %s" % (type(e).__name__, e)     # or the other ranks block in it
        statuses = _dist.all_gather_objects(status)
        fatal = [x[6:] for x in statuses if x.startswith("fatal:")]
        if fatal:
            raise RuntimeError("reading %s failed on a rank: %s" % (path, fatal[0]))
        if "boundary" not in statuses:
            # (after a boundary inside a quoted cell the NEXT rank starts mid-cell and sees a
            # malformed row: its error means nothing, the whole-file read below decides)
            errs = [x[6:] for x in statuses if x.startswith("error:")]
            if errs:
                raise io_native.GpaError(errs[0])    # a malformed row: every rank leaves together
            header, meta_rows, bits, kept = part
            bits, counts = _dist.all_gather_host_rows(bits)
            meta_rows = [row for rows in _dist.all_gather_objects(meta_rows) for row in rows]
            log.info("Read the gene presence/absence file in %d byte ranges (rows per rank: %s)"
                     % (world, ", ".join(str(c) for c in counts)))
            return header, meta_rows, bits, kept
    return io_native.read_gpa(path, delimiter, startcol, allowed_isolates, need_cols=wanted)


def _reduced_name(outdir, time):
    return "%sgene_presence_absence_reduced%s.csv" % (outdir, time)


def ReduceSet(genefile, delimiter, grabcols, startcol=14, allowed_isolates=None, time="",
              outdir="./"):
    """-r/-w: write the column subset of the table (methods.py:510-544)."""
    reader = csv.reader(genefile, skipinitialspace=True, delimiter=delimiter)
    header = next(reader)
    cols = list(range(startcol)) + [c for c in range(len(header)) if header[c] in allowed_isolates]
    log.info("Writing gene presence absence file for the reduced set of isolates")
    name = _reduced_name(outdir, time)
    with open(name, "w") as out:
        w = csv.writer(out, delimiter=delimiter)
        w.writerow([header[c] for c in cols])
        for r in reader:
            w.writerow([r[c] for c in cols])
    log.info("Finished writing reduced gene presence absence list to file %s" % name)
    return name


def Csv_to_dic(csvfile, delimiter, allowed_isolates, strains):
    """Read the traits table (methods.py:546-614): returns (traitsdic, Prunedic);
    isolates with a missing value are dropped from that trait only."""
    cols = list(zip(*csv.reader(csvfile, delimiter=delimiter)))
    if len(cols) < 2:
        sys.exit("Please check that your traits file is formatted properly and contains at "
                 "least one trait")
    traitsdic, prunedic = {}, {}
    for tcol in cols[1:]:
        p = dict(zip(cols[0], tcol))
        if "" in p:
            name = p.pop("")
        elif "Name" in p:
            name = p.pop("Name")
        else:
            sys.exit("Make sure the top-left cell in the traits file is either empty or "
                     "'Name'. Do not include empty rows")
        if allowed_isolates is not None:
            p = {s: v for s, v in p.items() if s in allowed_isolates}
        if not all(v in ALLOWED_TRAIT for v in p.values()):
            sys.exit("Unrecognized character found in trait file. Allowed values (no "
                     "commas): %s" % ",".join(["0", "1", "NA", ".", "-", " ", ""]))
        missing = [s for s, v in p.items() if v in MISSING_TRAIT]
        if missing:
            log.warning("WARNING: Some isolates have missing values for trait %s. "
                        "Missing-value isolates will not be counted in association analysis "
                        "towards this trait." % str(name))
        kept = {s: v for s, v in p.items() if v not in MISSING_TRAIT} if missing else p
        prune = list(missing)
        if not all(s in p for s in strains):
            log.error("ERROR: Some isolates in your gene presence absence file were not "
                      "represented in your traits file. These will count as MISSING data and "
                      "will not be included.")
            prune += [s for s in strains if s not in p and s not in prune]
        traitsdic[name] = kept
        prunedic[name] = prune + [None]
    return traitsdic, prunedic


# ---------------------------------------------------------------------------
# Statistics
# ---------------------------------------------------------------------------
def _as_table(genedic):
    return genedic if isinstance(genedic, GeneTable) else GeneTable.from_genedic(genedic)


def Perform_statistics(traits, genes):
    """One (gene, trait) table (methods.py:930-982): ``traits`` {strain: "0"/"1"},
    ``genes`` {strain: 0/1, ...}.  Counted on the GPU through the same kernel as
    the batched path."""
    strains = list(traits.keys())
    for s in strains:
        if s not in genes:
            log.critical("CRITICAL: Could not find %s in the genes file." % str(s))
            sys.exit("Make sure strains are named the same in your traits file as in your "
                     "gene presence/absence file")
    g = np.array([[1 if genes[s] else 0 for s in strains]], dtype=np.uint8)
    t = np.array([[2 if traits[s] in ("NA", "-", ".") else int(traits[s]) for s in strains]],
                 dtype=np.uint8)
    eng = get_engine()
    N = len(strains)
    counts, _ = eng.counts(eng.pack_dense(g), eng.vecrows(pack_bits_rows(t == 1), N),
                           eng.vecrows(pack_bits_rows(t != 2), N))
    tpgp, tpgn, tngp, tngn = (int(x) for x in counts.cpu().numpy()[0, 0])
    gene_trait = {}
    for j, s in enumerate(strains):
        gene_trait[s] = "NA" if t[0, j] == 2 else \
            ("A" if g[0, j] else "a") + ("B" if t[0, j] == 1 else "b")
    pattern = "".join(str(int(x)) for x in g[0])
    return {"statistics": {"tpgp": tpgp, "tpgn": tpgn, "tngp": tngp, "tngn": tngn},
            "hash": int(pattern, 2) if pattern else 0, "gene_trait": gene_trait}


def bonferroni_bh(p_sorted_input, number_of_tests, order=None):
    """Bonferroni and step-up Benjamini-Hochberg exactly as methods.py:903-925.

    ``p_sorted_input``: p-values in insertion order.  The reference sorts
    stably, keeps the least significant p as is, and walks towards the most
    significant with  bh = last if tie else min(last, p*ntests/rank), where
    tie = exact equality with the next sorted p.  Vectorised without changing
    a single floating-point operation: inside a run of equal p only the run's
    last (highest-rank) element evaluates min(); every other member copies it.
    So: reversed cumulative minimum over the run ends, broadcast to the runs.
    ``order``: the stable ascending argsort of the p-values if the caller already has it."""
    p = np.asarray(p_sorted_input, dtype=np.float64)
    n = p.shape[0]
    if n == 0:
        # the reference raises IndexError at methods.py:914 here
        raise IndexError("no testable genes for this trait")
    order = np.argsort(p, kind="stable") if order is None else order
    sp = p[order]
    v = sp * number_of_tests / (np.arange(n, dtype=np.float64) + 1.0)
    v[n - 1] = sp[n - 1]
    is_end = np.ones(n, dtype=bool)
    is_end[:-1] = sp[:-1] != sp[1:]
    ends = np.nonzero(is_end)[0]
    bh_ends = np.minimum.accumulate(v[ends][::-1])[::-1]
    run = np.cumsum(is_end) - is_end
    bh = np.empty(n, dtype=np.float64)
    bh[order] = bh_ends[run]
    return np.minimum(p * number_of_tests, 1.0), np.minimum(bh, 1.0)


def _pattern_groups(table, maskrow, idx, hashes):
    """Group id per tested gene (``idx``): equal ids <=> identical presence
    pattern over the trait's valid isolates.  ``hashes``: (G, 2) uint64 from the
    device (scoary_row_hash); candidate groups are confirmed on the bit rows,
    so a hash collision only costs a second pass."""
    keyed = None
    if hashes is not None:
        h = hashes[idx]
        _, inv = np.unique(h, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        # confirm: within a hash group every row must equal the group's first row
        order = np.argsort(inv, kind="stable")
        gs = inv[order]
        first = np.nonzero(np.r_[True, gs[1:] != gs[:-1]])[0]
        rep = order[np.repeat(first, np.diff(np.r_[first, len(gs)]))]
        keyed = table.rows64[idx] & maskrow[None, :]
        if np.array_equal(keyed[order], keyed[rep]):
            return inv
    if keyed is None:
        keyed = table.rows64[idx] & maskrow[None, :]
    _, inv = np.unique(keyed, axis=0, return_inverse=True)
    return inv.reshape(-1)


# The optional per-gene columns of a --no_pairwise results file, in file order (after Empirical_p, which has the
# early-abort denominator and exists in pairwise mode too): (CSV name, key of its array in _associate's result,
# True = a count r, read as uint32 and written as (r + 1) / (P + 1); False = the value as it is).  The arrays
# reach the host beside the gathered records -- which is why their flags need a single process -- except r_fwer,
# which travels in the records' nstop word (--permute-fwer excludes early abort): so a sharded run gathers it.
OPTIONAL_COLUMNS = (
    ("Westfall_Young_p", "r_fwer", True),
    ("Westfall_Young_stepdown_p", "r_fwer_sd", True),
    ("CMH_p", "cmh_p", False),
    ("CMH_odds_ratio", "cmh_odds", False),
    ("CMH_empirical_p", "r_cmh", True),
    ("CMH_Westfall_Young_p", "r_cmh_fwer", True),
    ("CMH_Westfall_Young_stepdown_p", "r_cmh_fwer_sd", True),
    ("CMH_exact_p", "cmh_exact_p", False),
    ("CMH_exact_odds_ratio", "cmh_exact_odds", False),                  # --cmh-exact-odds (spec S13): these three
    ("CMH_exact_odds_ratio_lower", "cmh_exact_odds_lower", False),
    ("CMH_exact_odds_ratio_upper", "cmh_exact_odds_upper", False),
)
# --cmh-homogeneity (spec S14): its column is written after every column above
HOMOGENEITY_COLUMNS = (("CMH_homogeneity_p", "cmh_homog_p", False),)
DEFAULT_EXACT_LEVEL = 0.95          # --cmh-exact-level

# The rules of the flags behind them, in the order they are checked (which decides the message a faulty run sees
# first, and is not the columns' order).  kw: the Setup_results keyword; sentence: what follows "needs
# --no_pairwise"; one_rank: why the flag needs a single rank, or None; needs_cmh: the key of the RULE_TEXT entry that
# reports a run without --cmh FILE, or None where the flag does not need it.
FlagRule = namedtuple("FlagRule", "flag kw sentence needs_permutations no_early_abort one_rank needs_cmh")
FLAG_RULES = (
    FlagRule("--permute-fwer", "fwer", "The Westfall-Young minima are taken over the Fisher statistic of every gene",
             True, True, None, None),
    FlagRule("--permute-fwer-stepdown", "fwer_stepdown",
             "The Westfall-Young minima are taken over the Fisher statistic of every gene", True, True,
             "the successive minima run over all genes in one order; gene shards do not compose", None),
    FlagRule("--cmh", "cmh", "The Cochran-Mantel-Haenszel test is a test of every gene, beside Fisher's", False, True,
             "its results reach the host beside the gathered records of a single process", None),
    FlagRule("--permute-strata", "strata", "The strata restrict the permutations of the Fisher statistic", True, False,
             None, None),
    FlagRule("--cmh-fwer", "cmh_fwer", "The Westfall-Young minima are taken over the Cochran-Mantel-Haenszel statistic "
             "of every gene", True, True, "its results reach the host beside the gathered records of a single process",
             "cmh"),
    FlagRule("--cmh-fwer-stepdown", "cmh_fwer_stepdown", "The Westfall-Young minima are taken over the "
             "Cochran-Mantel-Haenszel statistic of every gene", True, True,
             "the successive minima run over all genes in one order; gene shards do not compose", "cmh"),
    FlagRule("--cmh-exact-odds", "cmh_exact_odds", "The exact conditional odds ratio is an estimate for every gene "
             "over the strata, beside Fisher's test", False, False, "its results reach the host beside the gathered "
             "records of a single process", "cmh_exact"),
    FlagRule("--cmh-exact", "cmh_exact", "The exact conditional test is a test of every gene over the strata, beside "
             "Fisher's", False, False, "its results reach the host beside the gathered records of a single process",
             "cmh_exact"),
)
# --cmh-homogeneity: checked after every rule above; a single rank for --cmh's reason
HOMOGENEITY_RULES = (
    FlagRule("--cmh-homogeneity", "cmh_homogeneity", "The Breslow-Day test of homogeneity is a test of every gene over "
             "the strata, beside Fisher's", False, False,
             next(rule.one_rank for rule in FLAG_RULES if rule.flag == "--cmh"), "cmh_homogeneity"),
)
ALL_COLUMNS = OPTIONAL_COLUMNS + HOMOGENEITY_COLUMNS        # what every consumer of the two tables iterates
ALL_RULES = FLAG_RULES + HOMOGENEITY_RULES
# a broken rule as the command line reports it / as Setup_results raises it
RULE_TEXT = {
    "no_pairwise": ("Cannot use %(flag)s without --no_pairwise. %(why)s", None),
    "permutations": ("Cannot use %(flag)s without performing permutations. Use '--permute X' where X is a number "
                     "equal to or larger than 10",
                     "%(kw)s needs the Fisher-statistic permutations of --no_pairwise (permutations >= 10)"),
    "early_abort": ("Cannot use %(flag)s together with --permute-early-abort. Every gene has to see every "
                    "permutation", "%(kw)s excludes early_abort"),
    "cmh": ("Cannot use %(flag)s without --cmh FILE. The minima are taken over the statistic of the "
            "Cochran-Mantel-Haenszel test over the strata of FILE", "%(kw)s needs cmh (and its strata)"),
    "cmh_exact": ("Cannot use %(flag)s without --cmh FILE. The exact test is taken over the strata of FILE",
                  "%(kw)s needs cmh (and its strata)"),
    "cmh_homogeneity": ("Cannot use %(flag)s without --cmh FILE. The odds ratios are compared across the strata of "
                        "FILE", "%(kw)s needs cmh (and its strata)"),
    "ranks": ("Cannot use %(flag)s under more than one rank: %(why)s", "%(kw)s needs a single process: %(why)s"),
}


def _broken_rules(rule, no_pairwise, permutations, early_abort, files=None, cmh=False):
    """The messages of the rules of one row of ALL_RULES that a run breaks, in the order they are reported.
    ``files``: the messages of the command line's checks of the flag's own file, which come before the rank rule
    (() for a flag without one); None: the run is Setup_results' and the messages are its ValueErrors.  ``cmh``: the
    run has --cmh FILE / cmh=True."""
    def text(what, why=None):
        return RULE_TEXT[what][files is None] % {"flag": rule.flag, "kw": rule.kw, "why": why}
    if not no_pairwise:
        yield text("no_pairwise", rule.sentence)
    if rule.needs_permutations and permutations < 10:
        yield text("permutations")
    if rule.no_early_abort and early_abort:
        yield text("early_abort")
    if rule.needs_cmh and not cmh:
        yield text(rule.needs_cmh)
    yield from files or ()
    if rule.one_rank:
        from . import dist
        if dist.world_rank()[0] > 1:
            yield text("ranks", rule.one_rank)


def _associate(table, tarr, permutations=0, seed=DEFAULT_SEED, early_abort=False, strata=None, options=None):
    """Whole hot path for all traits; under torchrun (world > 1) every rank
    takes a stride gene shard (dist.GenePartition: the reference's domains,
    scoary/methods.py:1076-1078) and the per-gene records are all-gathered
    over RCCL and woven back into file order, so every rank returns the full arrays.
    ``early_abort``: the reference's sequential estimator (scoary/methods.py:1360-1363)
    on the Fisher statistic instead of the fixed-P count: out["nstop"] then holds the
    permutation count every gene stopped at (0 = ran to the end).
    ``strata``: the stratum index of every isolate of the table (--permute-strata): every permutation shuffles
    the labels within the strata only (spec S9); every rank generates the same labels.
    ``options``: Setup_results' ``active`` mapping with "cmh_exact_level" (None: nothing optional).  Its keys:
    ``fwer`` / ``fwer_stepdown``: the Westfall-Young results (engine.westfall_young, spec S7 / S8): out["minp"]
    [T, P] and out["r_fwer"] / out["r_fwer_sd"] [T, G].  Under gene sharding every rank takes the minima over its
    own genes and one all_reduce(MIN) of the [T, P] doubles precedes the count of r_fwer; the step-down counts do
    not compose over shards (single process only).
    ``cmh`` (needs ``strata``; single process, no early abort): the Cochran-Mantel-Haenszel test over the strata
    (spec S10): out["cmh_p"], out["cmh_odds"] [T, G] and, with permutations, out["r_cmh"].
    ``cmh_fwer`` / ``cmh_fwer_stepdown`` (need ``cmh`` and permutations): the Westfall-Young passes over the CMH
    statistic (spec S11): out["r_cmh_fwer"] / out["r_cmh_fwer_sd"] [T, G].
    ``cmh_exact`` (needs ``cmh``, not permutations): the exact conditional test over the strata (spec S12):
    out["cmh_exact_p"] [T, G].
    ``cmh_exact_odds`` (needs ``cmh``, not permutations): the conditional maximum-likelihood odds ratio over the strata
    and its exact confidence limits at ``cmh_exact_level`` (spec S13): out["cmh_exact_odds"],
    out["cmh_exact_odds_lower"], out["cmh_exact_odds_upper"] [T, G].
    ``cmh_homogeneity`` (needs ``cmh``, not permutations): the Breslow-Day test of homogeneity of the odds ratios over
    the strata with Tarone's correction (spec S14): out["cmh_homog_p"] [T, G].
    How each of these arrays reaches the host: ALL_COLUMNS."""
    import torch
    from . import dist
    opt = {**dict.fromkeys((rule.kw for rule in ALL_RULES), False), **(options or {})}
    eng = get_engine()
    G, N, T = len(table), len(table.strains), tarr.shape[0]
    with _stage("device setup (H2D, tiling, trait plan)"):
        trv = eng.vecrows(pack_bits_rows(tarr == 1), N)
        mkv = eng.vecrows(pack_bits_rows(tarr != 2), N)
        plan = eng.trait_plan(trv, mkv, N)            # margins + mask classes: once per trait set
        with_strata = strata is not None and (permutations > 0 or opt["cmh"])
        sp = eng.strata_plan(strata, trv, mkv, N) if with_strata else None

    def scipy_digits(res):
        # Up to 170 isolates k_fisher's p IS scipy.stats.fisher_exact's double; above, it is the exact value of SciPy's
        # rule to ~3e-15 -- inside the path's 1e-12, not the digits the reference writes.  What gets PRINTED is
        # therefore passed through scoary_fisher_scipy (Boost's prime-factorised pmf restated, bit for bit SciPy up
        # to 104 723 isolates): the result files are the reference's bytes at any realistic size.  An
        # output-fidelity pass, ~50 x k_fisher per table (9.5 ms per 500 000 tables at N = 2000) and not part of the
        # step bench.py times; SCOARY_FISHER_SCIPY=0 keeps k_fisher's value.
        if N <= 170 or os.environ.get("SCOARY_FISHER_SCIPY", "1") == "0":
            return
        with _stage("SciPy's digits for the printed p (k_fisher_scipy)"):
            skipped = eng.fisher_scipy(res["counts"], res["p"])
            torch.cuda.synchronize(eng.device)
        if skipped:
            log.info("%d tables are outside what scoary_fisher_scipy takes (more than %d isolates): their p is the exact "
                     "value of SciPy's rule (within 1e-12 of SciPy), not SciPy's last digits"
                     % (skipped, eng.fisher_scipy_max_isolates()))

    def local(sel):
        a = sel.start
        whole = sel == slice(0, G, 1)
        if len(range(*sel.indices(G))) == 0:
            if opt["fwer"]:     # a rank without genes still takes part in the reduction of the minima
                beside["minp"] = dist.all_reduce_min(torch.ones((T, permutations), dtype=torch.float64,
                                                                device=eng.device))
            return torch.zeros((T, 0, dist.REC_WORDS), dtype=torch.int32, device=eng.device)
        with _stage("device setup (H2D, tiling, trait plan)"):
            gm = table.on_device(eng) if whole else eng.tile_rows(table.rows64[sel], N)
            torch.cuda.synchronize(eng.device)
        if permutations > 0 and not early_abort and gm.lists is None and eng.lists_supported(N):
            # list-driven permutation kernel: cost follows each gene's minority count.  The
            # index array (4 bytes per padded minority entry, 2 for N > 20479) is sized by the
            # plan before it is allocated: a wide, dense matrix that would not fit keeps the
            # dense kernels (same results, no lists) instead of dying in the allocator
            from .engine import ListMemoryError
            try:
                with _stage("index lists (device)"):
                    eng.build_lists(gm)
                    torch.cuda.synchronize(eng.device)
            except (ListMemoryError, torch.cuda.OutOfMemoryError) as e:
                gm.lists = None
                log.info("index lists not built (%s); using the dense permutation kernels" % e)
        elif permutations > 0 and not early_abort and not eng.lists_supported(N) and a == 0:
            # more than 131 070 isolates: the list counts would need a 17th counter plane; the
            # dense AND + popcount kernels take over (same results, 1.5-3x the time per test)
            log.info("%d isolates: more than the list-driven permutation kernel takes (%d); "
                     "using the dense permutation kernels" % (N, eng.lib.scoary_list_max_isolates()))
        if early_abort and permutations > 0:
            from . import tree as T_
            res = eng.associate(gm, trv, mkv, permutations=0, plan=plan)
            crit = eng.fisher(res["counts"], want_crit=True)[2]
            scipy_digits(res)
            r, nstop = eng.permute_sequential(gm, mkv, res["margins"], crit, permutations, seed,
                                              T_._abort_thresholds(permutations), strata=sp)
            res["r"] = r
            return eng.pack_records(res, nstop=nstop)
        with _stage("kernels (counts, Fisher, permutations)"):
            res = eng.associate(gm, trv, mkv, permutations=permutations, seed=seed, plan=plan, strata=sp,
                                cmh=opt["cmh"], cmh_exact=opt["cmh_exact"], cmh_exact_odds=opt["cmh_exact_odds"],
                                cmh_exact_level=opt.get("cmh_exact_level", DEFAULT_EXACT_LEVEL),
                                cmh_homogeneity=opt["cmh_homogeneity"])
            torch.cuda.synchronize(eng.device)
        beside.update({key: res[key] for _name, key, _count in ALL_COLUMNS if key in res})
        if opt["fwer"] or opt["fwer_stepdown"]:
            with _stage("Westfall-Young step-down minP (p tables, k_stepdown_minp)" if opt["fwer_stepdown"] else
                        "Westfall-Young minP (p tables, k_permute_minp)"):
                # before the SciPy-digits pass rewrites the last ulp of p (westfall_young)
                beside.update(eng.westfall_young(gm, trv, mkv, permutations, seed, res, opt["fwer"],
                                                 opt["fwer_stepdown"], strata=sp, reduce=dist.all_reduce_min))
                torch.cuda.synchronize(eng.device)
        if opt["cmh_fwer"] or opt["cmh_fwer_stepdown"]:
            with _stage("Westfall-Young minP of the CMH statistic (tables, %s)"
                        % ("k_stepdown_minp" if opt["cmh_fwer_stepdown"] else "k_permute_minp")):
                beside.update(eng.westfall_young(gm, trv, mkv, permutations, seed, res, strata=sp,
                                                 cmh_fwer=opt["cmh_fwer"], cmh_stepdown=opt["cmh_fwer_stepdown"]))
                torch.cuda.synchronize(eng.device)
        scipy_digits(res)
        with _stage("kernels (counts, Fisher, permutations)"):
            rec = eng.pack_records(res, nstop=beside.pop("r_fwer", None))
            torch.cuda.synchronize(eng.device)
        return rec

    beside = {}         # the device arrays that reach the host beside the gathered records (ALL_COLUMNS)
    rec = dist.associate_sharded(local, G)
    with _stage("results D2H"):
        # the stable p order for BH: numpy does 200 000 doubles in 25-40 ms, which beats the
        # first-use cost of torch's sort kernels in a fresh process (0.2-0.4 s of lazy code loading,
        # profiles/r05_e2e_cli_*); the traits' sorts also run on worker threads (Setup_results), so
        # the device sort only wins from tens of millions of (gene, trait) pairs on
        p_order = _p_order_on_device(rec) if T * G >= DEVICE_SORT_MIN_PAIRS else None
        out = dist.numpy_records(rec)
        out["p_order"] = p_order
    if permutations <= 0:
        out["r"] = None
    if opt["fwer"]:
        out["r_fwer"], out["nstop"] = out["nstop"], np.zeros_like(out["nstop"])
    if opt["fwer_stepdown"]:
        out["r_fwer_sd"] = np.zeros((T, 0), dtype=np.int32)         # (a table without genes)
    for key in ("minp",) + tuple(key for _name, key, _count in ALL_COLUMNS):
        if key in beside:
            out[key] = beside[key].cpu().numpy()
    return out


DEVICE_SORT_MIN_PAIRS = 32_000_000
HOST_THREADS_MIN_PAIRS = 200_000        # (gene, trait) pairs from which the per-trait statistics use worker threads


def _p_order_on_device(rec):
    """Per trait: the testable genes (skip rule, methods.py:804-814) in ascending order of their
    Fisher p, ties in file order -- the stable sort Benjamini-Hochberg (methods.py:903-925) and
    the results writer (:1124) both start from.  The records are still on the device here, so the
    one O(G log G) step of the host statistics is one batched torch.argsort there (a stable sort
    of 200 000 doubles is 25-40 ms per trait in numpy, 50 traits x 1 M genes would be a minute).
    Returns a list of int64 arrays of positions into the trait's testable genes."""
    torch = _torch_mod()
    T, G, _ = rec.shape
    if G == 0:
        return [np.zeros(0, dtype=np.int64) for _ in range(T)]
    r = rec.contiguous()
    c = r[:, :, 0:4]
    testable = ((c[:, :, 0] + c[:, :, 2]) != 0) & ((c[:, :, 1] + c[:, :, 3]) != 0)
    pv = r[:, :, 4:6].reshape(-1).clone().view(torch.float64).view(T, G)
    key = torch.where(testable, pv, torch.full_like(pv, float("inf")))
    order = torch.argsort(key, dim=1, stable=True).to(torch.int32).cpu().numpy()
    tst = testable.cpu().numpy()
    out = []
    for t in range(T):
        n = int(tst[t].sum())
        pos = np.cumsum(tst[t]) - 1                       # gene index -> position among the testable
        out.append(pos[order[t, :n]].astype(np.int64))
    return out


def _torch_mod():
    import torch
    return torch


def _usable_cpus():
    """Logical CPUs this process may use: the affinity mask and the cgroup quota applied to
    os.cpu_count() (a container is often granted far fewer than the host has)."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()
        if quota != "max":
            n = min(n, max(1, int(float(quota) / float(period))))
    except (OSError, ValueError):
        pass
    return max(1, n)


def Setup_results(genedic, traitsdic, collapse, permutations=0, seed=DEFAULT_SEED,
                  early_abort=False, fwer=False, fwer_stepdown=False, strata=None, cmh=False, cmh_fwer=False,
                  cmh_fwer_stepdown=False, cmh_exact=False, cmh_exact_odds=False, cmh_exact_level=0.95,
                  cmh_homogeneity=False):
    """Counts, Fisher's exact test and B/BH correction for every trait x gene
    (methods.py:757-928).  ``permutations`` >= 10 additionally attaches the
    Fisher-statistic ``Empirical_p`` (= (r+1)/(P+1), methods.py:1365) to every
    row -- the north_star's replacement for the tree-statistic Permute loop.  ``fwer`` (with
    permutations): also ``Westfall_Young_p`` = (r_fwer+1)/(P+1), the single-step minP adjusted p.
    ``fwer_stepdown`` (with permutations, one process): also ``Westfall_Young_stepdown_p`` = (r_sd+1)/(P+1), the
    step-down minP adjusted p (spec S8).  ``strata`` (with permutations): one stratum index per isolate, in
    the table's strain order -- the permutations shuffle the labels within the strata only (spec S9), which
    changes the values of Empirical_p and of the Westfall-Young columns and nothing else.  ``cmh`` (needs
    ``strata``, not permutations; one process, no early abort): also ``CMH_p`` and ``CMH_odds_ratio``, the
    Cochran-Mantel-Haenszel test and the Mantel-Haenszel common odds ratio over the strata (spec S10), and with
    permutations ``CMH_empirical_p`` = (r_cmh+1)/(P+1), the exact permutation p of that statistic.
    ``cmh_fwer`` / ``cmh_fwer_stepdown`` (with ``cmh`` and permutations): also ``CMH_Westfall_Young_p`` =
    (r_cmh_fwer+1)/(P+1) and ``CMH_Westfall_Young_stepdown_p`` = (r_cmh_fwer_sd+1)/(P+1), the single-step and
    step-down family-wise adjusted p of the CMH statistic under the within-stratum shuffles (spec S11).
    ``cmh_exact`` (with ``cmh``, not permutations; one process): also ``CMH_exact_p``, the two-sided exact conditional
    p over the strata (spec S12; R's mantelhaen.test(exact = TRUE), Fisher's exact test when there is one stratum).
    ``cmh_exact_odds`` (with ``cmh``, not permutations; one process): also ``CMH_exact_odds_ratio``,
    ``CMH_exact_odds_ratio_lower`` and ``CMH_exact_odds_ratio_upper``, the conditional maximum-likelihood estimate of
    the common odds ratio and its exact confidence limits at ``cmh_exact_level`` (spec S13; the estimate and conf.int
    of the same R test).
    ``cmh_homogeneity`` (with ``cmh``, not permutations; one process): also ``CMH_homogeneity_p``, the p of the
    Breslow-Day test of homogeneity of the odds ratios over the strata with Tarone's correction (spec S14; R's
    DescTools::BreslowDayTest(correct = TRUE)), written after every other column."""
    if cmh and strata is None:
        raise ValueError("cmh needs strata")
    # (permutations are 0 here whenever the run is not --no_pairwise; with cmh the strata are its own)
    active = {"fwer": fwer, "fwer_stepdown": fwer_stepdown, "cmh": cmh, "strata": strata is not None and not cmh,
              "cmh_fwer": cmh_fwer, "cmh_fwer_stepdown": cmh_fwer_stepdown, "cmh_exact": cmh_exact,
              "cmh_exact_odds": cmh_exact_odds, "cmh_homogeneity": cmh_homogeneity}
    if cmh_exact_odds and not 0.0 < float(cmh_exact_level) < 1.0:
        raise ValueError("cmh_exact_level must lie inside (0, 1), not %r" % (cmh_exact_level,))
    for rule in (rule for rule in ALL_RULES if active[rule.kw]):
        for text in _broken_rules(rule, True, permutations, early_abort, cmh=cmh):
            raise ValueError(text)
    table = _as_table(genedic)
    names, tarr = _trait_arrays(traitsdic, table.strains)
    if strata is not None and len(strata) != len(table.strains):
        raise ValueError("strata: one stratum index per isolate of the gene table")
    dev = _associate(table, tarr, permutations if permutations >= 10 else 0, seed, early_abort, strata,
                     {**active, "cmh_exact_level": cmh_exact_level})
    collapse_hashes = None
    if collapse:
        eng = get_engine()
        N = len(table.strains)
        collapse_hashes = eng.row_hash(table.on_device(eng),
                                       eng.vecrows(pack_bits_rows(tarr != 2), N))
    all_traits, combos = {}, {}
    G = len(table)
    t_host = _time.perf_counter()

    def one_trait(t):
        trait = names[t]
        c = dev["counts"][t]                                   # tpgp, tpgn, tngp, tngn
        testable = ((c[:, 0] + c[:, 2]) != 0) & ((c[:, 1] + c[:, 3]) != 0)
        number_of_tests = G - int((~testable).sum())
        idx = np.nonzero(testable)[0]
        if len(idx) == 0:
            # (the reference falls over here too: IndexError from its empty sort list, scoary/methods.py:903-925)
            raise IndexError("Trait %s has no testable genes" % trait)
        p_all, or_all = dev["p"][t], dev["odds"][t]
        emp = None
        if dev["r"] is not None:
            # (r+1)/(P+1), :1365; with --permute-early-abort a gene that stopped after n
            # permutations gets (r+1)/(n+1) = the reference's (r+1.0)/(i+2.0), :1362
            n_used = np.where(dev["nstop"][t] > 0, dev["nstop"][t], permutations).astype(np.float64)
            emp = (dev["r"][t].astype(np.float64) + 1.0) / (n_used + 1.0)

        if not collapse:
            # names stay in the GeneTable: the result rows are (table, idx) -- nothing per
            # (gene, trait) is materialised in Python (a cfg5-sized run has 50 M such pairs)
            rows_idx, members, names_out = idx, None, None
            nugn = ann = None
            plist = p_all[idx]
            bh_rank_p = plist
        else:
            # identical presence pattern over the trait's valid isolates => one
            # merged unit (methods.py:816-840).  In the reference's dict
            # bookkeeping a unit is re-inserted (at the end) whenever it absorbs a
            # gene and takes that gene's statistics, so: unit order = ascending
            # index of its LAST member; name / NUGN / annotation = members joined
            # by "--" in file order; statistics of the last member.
            maskrow = pack_bits_rows((tarr[t:t + 1] != 2))[0]
            group = _pattern_groups(table, maskrow, idx, collapse_hashes[t] if
                                    collapse_hashes is not None else None)
            order_g = np.argsort(group, kind="stable")           # members stay in file order
            gs = group[order_g]
            starts = np.nonzero(np.r_[True, gs[1:] != gs[:-1]])[0]
            ends = np.r_[starts[1:], len(gs)]
            last_pos = order_g[ends - 1]                         # position (in idx) of last member
            unit_order = np.argsort(last_pos, kind="stable")
            members_idx = [idx[order_g[starts[u]:ends[u]]].tolist() for u in unit_order]
            number_of_tests -= int(len(idx) - len(starts))
            rows_idx = np.array([m[-1] for m in members_idx], dtype=np.int64)
            members = [[table.ids[i] for i in m] for m in members_idx]
            names_out = ["--".join(m) for m in members]
            nugn = ["--".join(table.nugn[i] for i in m) for m in members_idx]
            ann = ["--".join(table.annotation[i] for i in m) for m in members_idx]
            plist = p_all[rows_idx]
            # the reference's p_value_list keeps one entry per tested gene,
            # superseded names included (methods.py:873/892), so BH ranks count
            # them; a unit's BH is that of its last member's entry
            bh_rank_p = p_all[idx]
            bh_entry = last_pos[unit_order]

        cc = c[rows_idx]
        num_pos = (cc[:, 0] + cc[:, 1]).astype(np.float64)
        num_neg = (cc[:, 2] + cc[:, 3]).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            sens = np.where(num_pos > 0, cc[:, 0].astype(np.float64) / num_pos * 100, 0.0)
            spes = np.where(num_neg > 0, cc[:, 3].astype(np.float64) / num_neg * 100, 0.0)
        # stable ascending order of the testable genes' p: from the device if it came along
        p_order = dev["p_order"][t] if dev.get("p_order") is not None else None
        if not collapse:
            if p_order is None:
                p_order = np.argsort(plist, kind="stable")
            B, BH = bonferroni_bh(plist, number_of_tests, order=p_order)   # order shared with the writer
        else:
            _, bh_all = bonferroni_bh(bh_rank_p, number_of_tests, order=p_order)
            p_order = None                                   # the units' own p order is the writer's business
            BH = bh_all[bh_entry]
            B = np.minimum(plist * number_of_tests, 1.0)
        cols = {"tpgp": cc[:, 0], "tngp": cc[:, 2], "tpgn": cc[:, 1], "tngn": cc[:, 3],
                "sens": sens, "spes": spes, "OR": or_all[rows_idx], "p_v": plist,
                "B_p": B, "BH_p": BH}
        if emp is not None:
            cols["Empirical_p"] = emp[rows_idx]
        for name, key, count in ALL_COLUMNS:
            if key in dev:
                v = dev[key][t][rows_idx]
                cols[name] = (v.view(np.uint32).astype(np.float64) + 1.0) / (permutations + 1.0) if count else v
        if collapse:
            tr = TraitResults(names_out, nugn, ann, cols, number_of_tests, members)
        else:
            tr = TraitResults(None, None, None, cols, number_of_tests, None, table=table, rows_idx=rows_idx)
            tr.p_order = p_order
        return tr, GeneTraitCombinations(table, tr, members, tarr[t], t)

    for trait in names:
        log.info("Gene-wise counting and Fisher's exact tests for trait: %s" % str(trait))
    # the traits are independent and their statistics are numpy sorts / gathers that release the
    # interpreter lock: one worker thread per trait, as many as the process may use (50 traits x
    # 125 000 genes: 1.5 s one after the other)
    nthreads = min(len(names), _usable_cpus())
    if nthreads > 1 and G * len(names) >= HOST_THREADS_MIN_PAIRS:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=nthreads) as pool:
            done = list(pool.map(one_trait, range(len(names))))      # in trait order; the first error is re-raised
    else:
        done = [one_trait(t) for t in range(len(names))]
    for trait, (tr, gtc) in zip(names, done):
        all_traits[trait], combos[trait] = tr, gtc
    _stage.seconds["host statistics (skip rule, B / BH, columns)"] = \
        _stage.seconds.get("host statistics (skip rule, B / BH, columns)", 0.0) + _time.perf_counter() - t_host
    return {"Results": all_traits, "Gene_trait_combinations": combos}


def Permute(tree, GTC, permutations, cutoffs, seed=DEFAULT_SEED, trait_index=0):
    """Empirical p of ONE gene by label permutation (methods.py:1314-1369).

    With a ``tree`` (nested lists of the GTC's strains): the reference's
    statistic -- supporting (or opposing) pairs / max contrasting pairs of the
    PhyloTree, r = #permutations reaching the observed value, sequential early
    abort after 30 permutations, (r+1)/(P+1) otherwise.  With ``tree=None``: the
    Fisher statistic the north_star prescribes for the ``--no_pairwise`` path,
    (r+1)/(P+1) with r = #label shuffles whose 2x2 table is as or less probable
    than the observed one.  ``GTC`` is {strain: "AB"|"Ab"|"aB"|"ab"}."""
    if permutations < 10:
        sys.stdout.write("Number of permutations too few. The absolute minimum is 10.")
        return None
    strains = list(GTC.keys())
    g = np.array([[1 if GTC[s][0] == "A" else 0 for s in strains]], dtype=np.uint8)
    t = np.array([[1 if GTC[s][-1] == "B" else 0 for s in strains]], dtype=np.uint8)
    if tree is None:
        table = GeneTable(["gene"], [""], [""], strains, pack_bits_rows(g))
        dev = _associate(table, t, permutations, seed)
        return (float(dev["r"][0, 0]) + 1.0) / (permutations + 1.0)
    stage = _TreeStage(get_engine(), tree, strains, t[0], trait_index, seed)
    obs = stage.observed(pack_bits_rows(g))
    exceed = stage.permute(pack_bits_rows(g), obs, permutations)
    from .tree import empirical_p_sequential
    return empirical_p_sequential(exceed[0])


class _TreeStage:
    """Device state of the pairwise-comparison stage for ONE trait: the pruned
    tree as a stack program, label bits in tip order, and the kernels that
    evaluate genes (observed) and gene x permutation (scoary_tree_permute)."""

    def __init__(self, engine, tree, strains, trait_row, trait_index, seed):
        import torch
        from .tree import TreeProgram
        self.eng, self.N = engine, len(strains)
        self.trait_index, self.seed = int(trait_index), seed
        index_of = {s: i for i, s in enumerate(strains)}
        self.prog = TreeProgram(tree, index_of)
        dev = engine.device
        self.ops = torch.from_numpy(self.prog.ops).to(dev)
        self.tips = torch.from_numpy(self.prog.tips).to(dev)
        trait_row = np.asarray(trait_row, dtype=np.uint8)
        self.label_rows = engine.vecrows(pack_bits_rows((trait_row == 1)[None]), self.N)
        self.mask_rows = engine.vecrows(pack_bits_rows((trait_row != 2)[None]), self.N)
        self.labels_tip = engine.gather_bits(self.label_rows, self.tips)
        self.margins = torch.tensor([[int((trait_row == 1).sum()), int((trait_row != 2).sum())]],
                                    dtype=torch.int32, device=dev)

    def _gene_tip_bits(self, rows64):
        return self.eng.gather_bits(self.eng.vecrows(rows64, self.N), self.tips)

    def observed(self, rows64):
        """(G, 3) int32 numpy: max contrasting / supporting / opposing pairs."""
        gt = self._gene_tip_bits(rows64)
        out = self.eng.tree_pairs(self.ops, self.prog.depth, gt, self.labels_tip, self.prog.ntips)
        return out[:, 0, :].cpu().numpy()

    def permute(self, rows64, obs, permutations, batch_threads=1 << 26):
        """(G, P) uint8 numpy exceedance flags (methods.py:1353-1355) under the
        spec-S4 label permutations 0..P-1 of this trait."""
        import torch
        gt = self._gene_tip_bits(rows64)
        obs_d = torch.from_numpy(np.ascontiguousarray(obs, dtype=np.int32)).to(self.eng.device)
        G = gt.shape[0]
        out = np.empty((G, permutations), dtype=np.uint8)
        pb = max(1, min(permutations, batch_threads // max(G, 1)))
        for p0 in range(0, permutations, pb):
            nb = min(pb, permutations - p0)
            perms = self.eng.perm_generate(self.mask_rows, self.margins, self.N, nb, p0, self.seed,
                                           trait_base=self.trait_index)
            ptip = self.eng.gather_bits(perms[0], self.tips)
            ex = self.eng.tree_permute(self.ops, self.prog.depth, gt, ptip, self.prog.ntips, obs_d)
            out[:, p0:p0 + nb] = ex.cpu().numpy()
        return out


# ---------------------------------------------------------------------------
# Output
# ---------------------------------------------------------------------------
def _fmt(x):
    """str() of the reference's cells: ints as decimals, floats as Python's
    shortest round-trip repr."""
    if isinstance(x, (int, np.integer)):
        return str(int(x))
    return repr(float(x))


def SortResultsAndSetKey(genedic, key="p_v"):
    """{rank: gene} ascending by ``key``, stable (methods.py:1448-1454)."""
    if isinstance(genedic, TraitResults):
        order = np.argsort(np.asarray(genedic.column(key), dtype=np.float64), kind="stable")
        return {i: genedic.genes[j] for i, j in enumerate(order)}
    return {i: g for i, g in enumerate(sorted(genedic, key=lambda x: genedic[x][key]))}


CUT_FIELD = {"I": "p_v", "B": "B_p", "BH": "BH_p", "PW": "Plowest", "EPW": "Pboth",
             "P": "Empirical_p"}


def StoreResults(Results, max_hits, cutoffs, upgmatree, GTC, Prunedic, outdir, permutations,
                 num_threads, no_pairwise, genedic, extracolstoprint, firstcolnames, time="",
                 delimiter=",", seed=DEFAULT_SEED):
    def one(Trait, writer_threads=0):
        StoreTraitResult(Results[Trait], Trait, max_hits, cutoffs, upgmatree, GTC, Prunedic,
                         outdir, permutations, num_threads, no_pairwise, genedic,
                         extracolstoprint, firstcolnames, time, delimiter, seed=seed,
                         writer_threads=writer_threads)
    traits = list(Results)
    pairs = sum(len(Results[t]) for t in traits)
    nthreads = min(len(traits), _usable_cpus())
    if no_pairwise and nthreads > 1 and pairs >= HOST_THREADS_MIN_PAIRS:
        # --no_pairwise: a trait's file is sorting, filtering and formatting its own columns (numpy and
        # the native writer, both outside the interpreter lock) -- one worker thread per trait.  The
        # pairwise stage keeps the loop: it drives the GPU and logs its progress trait by trait.
        for Trait in traits:
            sys.stdout.write("\n")
            log.info("Storing results: " + Trait)
        from concurrent.futures import ThreadPoolExecutor
        with _stage("result files (sort, filter, pairwise stage, write)"):
            for Trait in traits:                     # the gene table's string columns: once, before the workers
                tr = Results[Trait]
                if isinstance(tr, TraitResults) and tr._table is not None:
                    _csv_text_columns(tr._table)
            with ThreadPoolExecutor(max_workers=nthreads) as pool:
                list(pool.map(lambda t: one(t, writer_threads=1), traits))   # the files are the parallel axis
        return
    for Trait in traits:
        sys.stdout.write("\n")
        log.info("Storing results: " + Trait)
        with _stage("result files (sort, filter, pairwise stage, write)"):
            one(Trait)


def decideifbreak(cutoffs, currentgene):
    """True when a gene violates a naive / Bonferroni / BH cutoff, which ends
    the pairwise stage for everything less significant (methods.py:1489-1508)."""
    for m in ("I", "B", "BH"):
        if m in cutoffs and currentgene[CUT_FIELD[m]] > cutoffs[m]:
            return True
    return False


def _kept_ranks(order, cols, cutoffs, num_threads=None):
    """Ranks (positions in ``order``) of the genes the reference's pairwise stage keeps.
    Worker k of n walks the ranks k, k+n, k+2n, ... and stops at ITS OWN first gene that fails
    an I/B/BH cutoff (scoary/methods.py:1076-1078, :1290-1294): the kept set is the union of the
    workers' prefixes.  With one worker, or with cutoff columns that are monotone in the rank,
    that is a prefix of ``order``; a non-monotone column (the stale-rank BH of --collapse) lets
    a later worker keep ranks past another worker's stop.  The weave's modulo (StoreTraitResult)
    is taken of these ranks."""
    nworkers = max(1, int(num_threads or 1))
    ranks = []
    for k in range(nworkers):
        for rank in range(k, len(order), nworkers):
            i = order[rank]
            if any(m in cutoffs and cols[CUT_FIELD[m]][i] > cutoffs[m] for m in ("I", "B", "BH")):
                break
            ranks.append(rank)
    return np.array(sorted(ranks), dtype=np.int64)


def _pairwise_stage(Trait, Traitname, order, cutoffs, upgmatree, GTC, Prunedic, permutations,
                    genedic, seed, num_threads=None):
    """PairWiseComparisons (methods.py:1208-1312) for the genes ``order`` (row
    indices, ascending naive p) of one trait, on the GPU: the prefix that passes
    the I/B/BH cutoffs gets max contrasting / supporting / opposing pairs, the
    two binomial p-values and, with permutations, the tree-statistic empirical p.
    Returns (row indices kept, their ranks in ``order``, dict of extra columns over those
    rows)."""
    from . import tree as T
    cols = {k: np.asarray(Trait.column(k)) for k in ("p_v", "B_p", "BH_p")}
    ranks = _kept_ranks(order, cols, cutoffs, num_threads)
    keep = np.asarray(order, dtype=np.int64)[ranks] if len(ranks) else np.zeros(0, dtype=np.int64)
    extra = {k: np.zeros(len(keep)) for k in ("Pbest", "Pworst", "Plowest", "Pboth")}
    for k in ("max_total_pairs", "max_propairs", "max_antipairs"):
        extra[k] = np.zeros(len(keep), dtype=np.int64)
    if permutations >= 10:
        extra["Empirical_p"] = np.zeros(len(keep))
    if len(keep) == 0:
        return keep, ranks, extra
    gtc = GTC[Traitname]
    table = gtc.table
    tree = upgmatree
    if len(Prunedic[Traitname]) > 0:
        tree = T.prune_missing(upgmatree, Prunedic[Traitname])
    stage = _TreeStage(get_engine(), tree, table.strains, gtc.trait_row, gtc.trait_index, seed)
    src = [Trait.source_index(i) if Trait.source_index(i) is not None else
           table.index(Trait.members[i][-1] if Trait.members is not None else Trait.gene_at(i))
           for i in keep]
    rows64 = table.rows64[src]
    obs = stage.observed(rows64)
    extra["max_total_pairs"] = obs[:, 0].astype(np.int64)
    extra["max_propairs"] = obs[:, 1].astype(np.int64)
    extra["max_antipairs"] = obs[:, 2].astype(np.int64)
    # the two binomial p-values of every gene (methods.py:1259-1275), SciPy's doubles (tree.binom_two_sided_many)
    tot, pro, anti = (obs[:, j].astype(np.int64) for j in range(3))
    both = T.binom_two_sided_many(np.concatenate([pro, tot - anti]), np.concatenate([tot, tot]))
    a, b = both[:len(keep)], both[len(keep):]
    best_is_a = pro >= anti
    extra["Pbest"], extra["Pworst"] = np.where(best_is_a, a, b), np.where(best_is_a, b, a)
    extra["Plowest"] = np.minimum(extra["Pbest"], extra["Pworst"])
    extra["Pboth"] = np.maximum(extra["Pbest"], extra["Pworst"])
    if permutations >= 10:
        log.info("Performing %d label permutations of the pairwise-comparison statistic for "
                 "%d genes on the GPU" % (permutations, len(keep)))
        exceed = stage.permute(rows64, obs, permutations)
        extra["Empirical_p"] = T.empirical_p_sequential_many(exceed)
    return keep, ranks, extra


def _csv_text_columns(table):
    """The three leading text cells of every gene of a GeneTable as string tables for the native
    writer, built once per table: Roary identifiers give (gene, non-unique name, annotation),
    identifiers of the form c0_|_c1_|_c2 (non-Roary files, scoary/methods.py:458-460) their three
    parts (methods.py:1154-1158).  None if some identifier splits into another number of cells
    (the general writer handles those)."""
    cached = getattr(table, "_csv_text", None)
    if cached is not None:
        return cached or None
    from . import io_native
    c0, c1, c2 = [], [], []
    for g, n, a in zip(table.ids, table.nugn, table.annotation):
        if "_|_" in g:
            parts = g.split("_|_")
            if len(parts) != 3:
                table._csv_text = False
                return None
            c0.append(parts[0]); c1.append(parts[1]); c2.append(parts[2])
        else:
            c0.append(g); c1.append(str(n)); c2.append(str(a))
    table._csv_text = tuple(io_native.TextColumn(c) for c in (c0, c1, c2))
    return table._csv_text


def _write_rows_native(fname, delimiter, header_line, Trait, table, sel_i, sel_k, colget, fields, extra, with_emp,
                       extracolstoprint, threads=0):
    """The rows of one results file through the native writer (scoary_results_write: string tables +
    index arrays + numeric columns, formatted by all cores) -- a -p 1.0 run of 50 traits x 125 000
    genes writes six million rows, 15-30 us each through the per-cell Python loop.  Returns False
    when the case is one the general writer keeps (--collapse units, exotic identifiers, no native
    library)."""
    from . import io_native
    if (not io_native.available() or os.environ.get("SCOARY_PY_WRITER") == "1" or len(delimiter) != 1
            or not delimiter.isascii() or Trait.members is not None or Trait._table is None or Trait._rows_idx is None):
        return False
    src = Trait._table
    text = _csv_text_columns(src)
    if text is None:
        return False
    tab_idx = np.asarray(Trait._rows_idx, dtype=np.int64)[sel_i]      # gene-table row of every written row
    text_cols, text_rows = list(text), [tab_idx, tab_idx, tab_idx]
    num = [np.asarray(colget[f])[sel_i] for f in fields]
    if extra is not None:
        num += [np.asarray(extra[k])[sel_k] for k in ("max_total_pairs", "max_propairs", "max_antipairs",
                                                      "Pbest", "Pworst")]
        if with_emp:
            num.append(np.asarray(extra["Empirical_p"])[sel_k])
    # grabbed input columns come after the numeric cells (methods.py:1190-1194): written as a second
    # block of text would break the column order, so those runs keep the general writer
    if extracolstoprint:
        return False
    io_native.results_write(fname, delimiter, header_line, text_cols, text_rows, num,
                            np.arange(len(sel_i), dtype=np.int64), threads=threads or _usable_cpus())
    return True


def _write_rows_python(fname, delimiter, header_line, Trait, table, sel_i, sel_k, colget, fields, extra, with_emp,
                       extracolstoprint):
    """The general writer: one Python string per cell (--collapse units, grabbed input columns)."""
    members = Trait.members
    with open(fname, "w") as out:
        out.write(header_line)
        for n, i in enumerate(sel_i):
            i = int(i)
            k = None if sel_k is None else int(sel_k[n])
            gene = Trait.gene_at(i)                     # only the rows that are written get names
            if "_|_" in gene:
                cells = gene.split("_|_")
            else:
                cells = [gene, str(Trait.nugn_at(i)), str(Trait.annotation_at(i))]
            cells += [_fmt(colget[f][i]) for f in fields]
            if extra is not None:
                cells += [_fmt(extra["max_total_pairs"][k]), _fmt(extra["max_propairs"][k]),
                          _fmt(extra["max_antipairs"][k]), _fmt(extra["Pbest"][k]),
                          _fmt(extra["Pworst"][k])]
                if with_emp:
                    cells.append(_fmt(extra["Empirical_p"][k]))
            for colname in extracolstoprint:
                key = colname + "_name"
                if "--" in gene:
                    parts = members[i] if members is not None else gene.split("--")
                    cells.append("--".join(str(table.extra[key][table.index(g)]) for g in parts))
                else:
                    cells.append(str(table.extra[key][table.index(gene)]))
            out.write(delimiter.join('"' + c + '"' for c in cells) + "\n")


def StoreTraitResult(Trait, Traitname, max_hits, cutoffs, upgmatree, GTC, Prunedic, outdir,
                     permutations, num_threads, no_pairwise, genedic, extracolstoprint,
                     firstcolnames, time="", delimiter=",", seed=DEFAULT_SEED, writer_threads=0):
    """Write ``<outdir><Trait><time>.results.csv`` (methods.py:1003-1197):
    header, rows sorted (stable) by the reference's key, every active cutoff
    applied, every cell double-quoted.  Without ``no_pairwise`` the
    pairwise-comparison stage runs first (see _pairwise_stage)."""
    permutations = int(permutations)
    fname = outdir + Traitname + time + ".results.csv"
    columns = list(firstcolnames) + [
        "Number_pos_present_in", "Number_neg_present_in", "Number_pos_not_present_in",
        "Number_neg_not_present_in", "Sensitivity", "Specificity", "Odds_ratio", "Naive_p",
        "Bonferroni_p", "Benjamini_H_p"]
    if not no_pairwise:
        columns += ["Max_Pairwise_comparisons", "Max_supporting_pairs", "Max_opposing_pairs",
                    "Best_pairwise_comp_p", "Worst_pairwise_comp_p"]
    with_emp = permutations >= 10
    if with_emp:
        columns.append("Empirical_p")
    if not isinstance(Trait, TraitResults):
        Trait = _trait_results_from_dict(Trait)
    # (a count has its denominator from the permutations: without them it is not written)
    optional = [name for name, _key, count in ALL_COLUMNS
                if no_pairwise and name in Trait.cols and (with_emp or not count)]
    columns += optional
    columns += list(extracolstoprint)
    table = _as_table(genedic) if extracolstoprint else None

    n = len(Trait)
    # (-m 0 or a negative -m: no rows, as the reference's xrange(num_results), :1024 / :1143)
    num_results = n if max_hits is None else max(0, min(max_hits, n))
    pcol = np.asarray(Trait.column("p_v"), dtype=np.float64)
    order = getattr(Trait, "p_order", None)
    if order is not None and len(order) == n and n > 1:
        # the order Setup_results already had -- valid only while the p column is the one it was
        # taken from (a caller may have replaced it): ascending, ties in row order, O(n) to check
        sp = pcol[order]
        if not np.all((sp[:-1] < sp[1:]) | ((sp[:-1] == sp[1:]) & (order[:-1] < order[1:]))):
            order = None
    if order is None or len(order) != n:
        order = np.argsort(pcol, kind="stable")
    order = order[:num_results]
    fields = ["tpgp", "tngp", "tpgn", "tngn", "sens", "spes", "OR", "p_v", "B_p", "BH_p"]
    if no_pairwise:
        log.info("Skipping population structure-aware analyses." if not with_emp else
                 "Performing %s label permutations per gene on the GPU (Fisher statistic)"
                 % permutations)
        cand = order
        colget = {k: np.asarray(Trait.column(k)) for k in fields}
        for k in (["Empirical_p"] if with_emp else []) + optional:
            colget[k] = np.asarray(Trait.column(k))
            fields.append(k)
        keyed = {CUT_FIELD[m]: colget[CUT_FIELD[m]] for m in cutoffs}
        sel = cand[np.all([keyed[CUT_FIELD[m]][cand] <= c for m, c in cutoffs.items()], axis=0)] \
            if cutoffs else cand
        rows = np.asarray(sel, dtype=np.int64)          # result rows to write, in order (no per-row objects)
        extra = None
    else:
        log.info("Calculating max number of contrasting pairs for each %s gene%s"
                 % ("significant" if with_emp else "nominally significant",
                    " and performing %d permutations" % permutations if with_emp else ""))
        keep, ranks, extra = _pairwise_stage(Trait, Traitname, order, cutoffs, upgmatree, GTC,
                                             Prunedic, permutations, genedic, seed, num_threads)
        colget = {k: np.asarray(Trait.column(k)) for k in fields}
        # sort key of the filtered set (methods.py:1124-1135); ``keep`` is already
        # in ascending-p order, and every sort is stable
        pos = np.arange(len(keep))
        if num_threads is not None and int(num_threads) > 1 and len(keep):
            # --threads n: the reference hands worker k the ranks k, k+n, k+2n, ... and weaves the
            # workers' results back thread by thread (scoary/methods.py:1076-1078, 1115-1122), so
            # rows with EQUAL sort keys come out in (rank mod n, rank) order
            # -- the modulo is of the gene's rank in the sorted results, not of its position in
            # ``keep`` (the two differ once a worker stopped before another)
            pos = np.lexsort((ranks, ranks % int(num_threads)))
        if any(m in cutoffs for m in ("I", "B", "BH")):
            pos = pos[np.argsort(colget["p_v"][keep][pos], kind="stable")]
        elif "EPW" in cutoffs:
            pos = pos[np.argsort(np.asarray(extra["Pboth"])[pos], kind="stable")]
        elif "PW" in cutoffs:
            pos = pos[np.argsort(np.asarray(extra["Plowest"])[pos], kind="stable")]
        elif "P" in cutoffs:
            pos = pos[np.argsort(np.asarray(extra["Empirical_p"])[pos], kind="stable")]
        else:
            log.info("No filtration applied")
        pos = pos[:min(num_results, len(keep))]
        rows = []
        for k in pos:
            i = int(keep[k])
            ok = True
            for m, c in cutoffs.items():
                f = CUT_FIELD[m]
                v = extra[f][k] if f in extra else colget[f][i]
                ok = ok and (v <= c)
            if ok:
                rows.append((i, int(k)))
    log.info("Storing results to file")
    sel_i = np.fromiter((r[0] for r in rows), dtype=np.int64, count=len(rows)) if not isinstance(rows, np.ndarray) \
        else rows
    sel_k = None if extra is None else np.fromiter((r[1] for r in rows), dtype=np.int64, count=len(rows))
    header_line = delimiter.join('"' + c + '"' for c in columns) + "\n"
    if not _write_rows_native(fname, delimiter, header_line, Trait, table, sel_i, sel_k, colget, fields, extra,
                              with_emp, extracolstoprint, threads=writer_threads):
        _write_rows_python(fname, delimiter, header_line, Trait, table, sel_i, sel_k, colget, fields, extra,
                           with_emp, extracolstoprint)
    return fname


def _trait_results_from_dict(rows):
    """Plain {gene: row dict} (the reference's Results[trait]) -> TraitResults."""
    genes = list(rows.keys())
    cols = {}
    for k in TraitResults.FIELDS + ("Empirical_p",) + tuple(name for name, _key, _count in ALL_COLUMNS):
        if genes and k in rows[genes[0]]:
            cols[k] = np.array([rows[g][k] for g in genes])
    return TraitResults(genes, [rows[g]["NUGN"] for g in genes],
                        [rows[g]["Annotation"] for g in genes], cols, len(genes))


def StoreUPGMAtreeToFile(upgmatree, outdir, time=""):
    """Write the tree as ``Tree<time>.nwk`` (methods.py:741-752)."""
    from .tree import newick_text
    name = str(outdir + ("Tree%s.nwk" % time))
    with open(name, "w") as f:
        f.write(newick_text(upgmatree) if upgmatree is not None else "None;")
    log.info("Wrote the UPGMA tree to file: %s" % name)
    return name


def filtrationoptions(cutoffs, collapse):
    long_names = {"I": "Individual (Naive)", "B": "Bonferroni", "BH": "Benjamini-Hochberg",
                  "PW": "Pairwise comparison (Best)", "EPW": "Pairwise comparison (Entire range)",
                  "P": "Empirical p-value (permutation-based)"}
    lines = ["-- Filtration options --"]
    lines += ["%s:    %s" % (long_names[k], v) for k, v in cutoffs.items()]
    lines.append("Collapse genes:    %s\n\n" % collapse)
    return lines


# ---------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------
def grabcoltype(string):
    """--include_input_columns: "4,6,8,16-23" / "ALL" -> 0-based column list
    (methods.py:1510-1549; ranges are half-open there, kept as is)."""
    if string == "ALL":
        return [-999]
    if string == "":
        return []
    cols = []
    for part in string.split(","):
        if "-" in part:
            try:
                ab = part.split("-")
                if not int(ab[1]) > int(ab[0]):
                    raise ValueError(part)
                cols += list(range(int(ab[0]), int(ab[1])))
            except (ValueError, TypeError, IndexError):
                sys.exit("Could not understand --include_input_columns argument %s" % part)
        else:
            # a word where a number belongs is a ValueError here as in the reference (which only catches TypeError,
            # :1537-1541): argparse turns it into its own "invalid grabcoltype value" error, exit status 2
            cols.append(int(part))
    cols = [c - 1 for c in cols if c - 1 not in (0, 1, 2)]
    if not all(c > 1 for c in cols):
        sys.exit("Could not understand --include_input_columns argument. Make sure all "
                 "numbers are positive and real.")
    return list(set(cols))


def ScoaryArgumentParser(argv=None):
    """Same flags, dests, types and defaults as methods.py:1551-1744, plus
    --seed for reproducible permutations."""
    ap = argparse.ArgumentParser(
        description="scoary_amd %s - MI355X-native pan-genome association "
                    "(Scoary %s compatible command line)" % (__version__, SCOARY_COMPAT_VERSION))
    g = ap.add_argument_group("Input options")
    g.add_argument("-t", "--traits", help="Trait table (csv): strains in rows, traits in "
                   "columns, 1 = trait present, 0 = absent, NA/./- = missing")
    g.add_argument("-g", "--genes", help="Gene presence/absence table (csv, Roary format); "
                   "strain names must match the trait table")
    g.add_argument("-n", "--newicktree", default=None,
                   help="Custom Newick tree for the pairwise-comparison stage")
    g.add_argument("-s", "--start_col", type=int, default=15,
                   help="1-based column where isolates start in the gene table (default 15)")
    g.add_argument("--delimiter", type=str, default=",",
                   help="Single-character cell delimiter of input and output files")
    g.add_argument("-r", "--restrict_to", help="File with a comma-separated list of isolates "
                   "to restrict the analysis to")
    o = ap.add_argument_group("Output options")
    o.add_argument("-o", "--outdir", default="./", help="Output directory (default .)")
    o.add_argument("-u", "--upgma_tree", action="store_true", default=False,
                   help="Write the calculated UPGMA tree to a newick file")
    o.add_argument("-p", "--p_value_cutoff", nargs="+", type=float, default=[0.05],
                   help="P-value cut-off(s): one for all correction methods or one per "
                   "method in -c order (default 0.05; 1.0 reports every gene)")
    o.add_argument("-c", "--correction", nargs="*", default=["I"],
                   choices=["I", "B", "BH", "PW", "EPW", "P"],
                   help="Filtration measures: I naive, B Bonferroni, BH Benjamini-Hochberg, "
                   "PW best pairwise, EPW entire pairwise range, P empirical (permutation)")
    o.add_argument("-m", "--max_hits", type=int, help="Report at most this many hits per trait")
    o.add_argument("--include_input_columns", dest="grabcols", type=grabcoltype, default=[],
                   help="Columns of the gene table to copy to the output, e.g. 4,6,8,16-23 or ALL")
    o.add_argument("-w", "--write_reduced", action="store_true", default=False,
                   help="With -r: also write the reduced gene presence/absence table")
    o.add_argument("--no-time", dest="no_time", action="store_true", default=False,
                   help="No timestamp in output file names")
    a = ap.add_argument_group("Analysis options")
    a.add_argument("-e", "--permute", type=int, default=0,
                   help="Number of trait-label permutations per gene for empirical p-values "
                   "(0 = off, minimum 10)")
    a.add_argument("--permute-early-abort", dest="permute_early_abort", action="store_true",
                   default=False,
                   help="With --no_pairwise --permute: use the reference's sequential estimator "
                   "with early abort for the Fisher-statistic permutations -- a gene stops after "
                   "i >= 30 permutations once 1 - binom.cdf(r, i, 0.1) < 0.05 and gets "
                   "(r+1)/(i+2) (large empirical p-values become coarse, like the reference's)")
    a.add_argument("--permute-fwer", dest="permute_fwer", action="store_true", default=False,
                   help="With --no_pairwise --permute: add the column Westfall_Young_p, the single-step "
                   "minP family-wise adjusted p -- (1 + number of permutations whose smallest Fisher p "
                   "over all genes is <= the gene's own p) / (permutations + 1) (scoary_amd extension)")
    a.add_argument("--permute-fwer-stepdown", dest="permute_fwer_stepdown", action="store_true", default=False,
                   help="With --no_pairwise --permute: add the column Westfall_Young_stepdown_p, the step-down "
                   "minP family-wise adjusted p -- every gene is compared, per permutation, with the smallest "
                   "Fisher p over the genes ranked at or behind it only; never above Westfall_Young_p, same "
                   "family-wise error (single process; scoary_amd extension)")
    a.add_argument("--permute-strata", dest="permute_strata", metavar="FILE", default=None,
                   help="With --no_pairwise --permute: shuffle the trait labels only within strata (lineage, "
                   "BAPS / PopPUNK cluster, sequence type, country ...), the permutation null for a structured "
                   "population. FILE is a CSV with a header row (read with --delimiter): column 1 the isolate "
                   "name, column 2 its stratum label; further columns are ignored. Changes Empirical_p and the "
                   "Westfall-Young columns (scoary_amd extension)")
    a.add_argument("--cmh", dest="cmh", metavar="FILE", default=None,
                   help="With --no_pairwise: the Cochran-Mantel-Haenszel test over the strata of FILE (the format of "
                   "--permute-strata): adds the columns CMH_p and CMH_odds_ratio (the Mantel-Haenszel common odds "
                   "ratio), the association inside the strata instead of across them. With --permute also "
                   "CMH_empirical_p, the exact permutation p of the CMH statistic, and every permutation then "
                   "shuffles the labels within these strata (single process; scoary_amd extension)")
    a.add_argument("--cmh-fwer", dest="cmh_fwer", action="store_true", default=False,
                   help="With --no_pairwise --cmh FILE --permute: add the column CMH_Westfall_Young_p, the single-step "
                   "family-wise adjusted p of the CMH statistic -- (1 + number of within-stratum permutations whose "
                   "largest CMH statistic over all genes is >= the gene's own) / (permutations + 1) (single process; "
                   "scoary_amd extension)")
    a.add_argument("--cmh-fwer-stepdown", dest="cmh_fwer_stepdown", action="store_true", default=False,
                   help="With --no_pairwise --cmh FILE --permute: add the column CMH_Westfall_Young_stepdown_p, the "
                   "step-down family-wise adjusted p of the CMH statistic -- every gene is compared, per permutation, "
                   "with the largest CMH statistic over the genes ranked at or behind it only; never above "
                   "CMH_Westfall_Young_p (single process; scoary_amd extension)")
    a.add_argument("--cmh-exact", dest="cmh_exact", action="store_true", default=False,
                   help="With --no_pairwise --cmh FILE: add the column CMH_exact_p, the two-sided exact conditional p "
                   "over the strata of FILE -- the pooled count against the convolution of the strata's "
                   "hypergeometric distributions, R's mantelhaen.test(exact = TRUE); needs no permutations; at most "
                   "8190 isolates (single process; scoary_amd extension)")
    a.add_argument("--cmh-exact-odds", dest="cmh_exact_odds", action="store_true", default=False,
                   help="With --no_pairwise --cmh FILE: add the columns CMH_exact_odds_ratio, CMH_exact_odds_ratio_lower "
                   "and CMH_exact_odds_ratio_upper, the conditional maximum-likelihood estimate of the common odds "
                   "ratio over the strata of FILE and its exact confidence limits -- the estimate and conf.int of R's "
                   "mantelhaen.test(exact = TRUE); needs no permutations and not --cmh-exact; at most 8190 isolates "
                   "(single process; scoary_amd extension)")
    a.add_argument("--cmh-homogeneity", dest="cmh_homogeneity", action="store_true", default=False,
                   help="With --no_pairwise --cmh FILE: add the column CMH_homogeneity_p, the p of the Breslow-Day test of "
                   "homogeneity of the odds ratios over the strata of FILE with Tarone's correction -- whether one "
                   "common odds ratio, CMH_odds_ratio, describes every stratum; R's DescTools::BreslowDayTest(correct = "
                   "TRUE); needs no permutations (single process; scoary_amd extension)")
    a.add_argument("--cmh-exact-level", dest="cmh_exact_level", type=float, default=None, metavar="FLOAT",
                   help="With --cmh-exact-odds: the confidence level of the limits, inside (0, 1) (default 0.95)")
    a.add_argument("--quantitative", dest="quantitative", metavar="FILE", default=None,
                   help="With --no_pairwise: FILE holds measured traits (isolates in rows, one named column per trait, "
                   "numbers in the cells, NA for missing), laid out like the traits file.  Every column is tested "
                   "against every gene with the Wilcoxon-Mann-Whitney rank-sum test (normal approximation with tie and "
                   "continuity corrections) and written to <trait>.ranksum.results.csv; --permute adds Empirical_p "
                   "from shuffles of the values over the isolates (single process; scoary_amd extension)")
    a.add_argument("--covariates", dest="covariates", metavar="FILE", default=None,
                   help="With --no_pairwise: FILE holds up to 8 numeric covariates (isolates in rows, one named column "
                   "per covariate, NA for missing), laid out like the --quantitative file: the axes of an MDS or PCA "
                   "of the core genome, sampling year, genome size.  Every trait of the traits file is tested against "
                   "every gene with the logistic score test next to them, written to <trait>.logistic.results.csv "
                   "with the one-step odds ratio; with --quantitative every measured trait gets the linear score "
                   "test (ordinary least squares' t test of the gene), written to <column>.linear.results.csv "
                   "(single process, no permutation columns; scoary_amd extension)")
    a.add_argument("--covariates-spa", dest="covariates_spa", action="store_true", default=False,
                   help="With --covariates: <trait>.logistic.results.csv gains four last columns, SPA_p (the "
                   "saddlepoint-corrected p of the score test: the normal approximation behind Score_p is weakest "
                   "for rare genes and unbalanced traits, where it can be too small by orders of magnitude), "
                   "SPA_Bonferroni_p and SPA_Benjamini_H_p over the same genes, and SPA_status (0: the score "
                   "chi-square is below the cutoff squared and SPA_p is Score_p; 1: the saddlepoint p; 2: none could be "
                   "formed and SPA_p is Score_p).  Rows stay sorted by Score_p and --max_hits still cuts by Score_p; "
                   "the linear files are untouched (scoary_amd extension)")
    a.add_argument("--covariates-spa-cutoff", dest="covariates_spa_cutoff", metavar="X", type=float, default=None,
                   help="With --covariates-spa: genes whose score statistic is below X standard deviations keep "
                   "Score_p (default %s, at least %s)" % (SCORE_SPA_CUTOFF, SCORE_SPA_MIN_CUTOFF))
    a.add_argument("--categorical", dest="categorical", metavar="FILE", default=None,
                   help="With --no_pairwise: FILE holds categorical traits (isolates in rows, one named column per "
                   "trait, any label in the cells, NA for missing), laid out like the traits file.  Every column of up "
                   "to 8 classes is tested against every gene with the Pearson chi-square test of the 2 x K table and "
                   "written to <trait>.categorical.results.csv with Cramer's V; --permute adds Empirical_p from "
                   "shuffles of the labels over the isolates (single process; scoary_amd extension)")
    a.add_argument("--categorical-strata", dest="categorical_strata", metavar="FILE", default=None,
                   help="With --categorical: FILE names a stratum (lineage, cluster) for every isolate, in the format "
                   "of --permute-strata. Adds the generalized Cochran-Mantel-Haenszel test of every gene against "
                   "each trait over the strata, written to <trait>.gcmh.results.csv; --permute adds Empirical_p "
                   "from label shuffles within the strata. The chi-square results stay as they are")
    a.add_argument("--categorical-fwer", dest="categorical_fwer", action="store_true", default=False,
                   help="With --categorical and --permute X (X >= 10): add the column Westfall_Young_p to the chi-square "
                   "results -- and, with --categorical-strata, to the generalized CMH results -- the single-step maxT "
                   "family-wise p over all genes of the table, from the same permutations that give Empirical_p "
                   "(single process; scoary_amd extension)")
    a.add_argument("--categorical-fwer-stepdown", dest="categorical_fwer_stepdown", action="store_true",
                   default=False,
                   help="With --categorical and --permute X (X >= 10): add the column Westfall_Young_stepdown_p to the "
                   "chi-square results -- and, with --categorical-strata, to the generalized CMH results -- the "
                   "step-down maxT family-wise p: a gene is compared with the genes at its rank and behind, so the p "
                   "is never above Westfall_Young_p (single process; scoary_amd extension)")
    a.add_argument("--quantitative-strata", dest="quantitative_strata", metavar="FILE", default=None,
                   help="With --quantitative: FILE names a stratum (lineage, cluster) for every isolate, in the format "
                   "of --permute-strata's file.  Every measured trait is additionally tested with the van Elteren "
                   "stratified rank-sum test -- ranks inside the strata, weights 1 / (n_s + 1) -- and written to "
                   "<trait>.vanelteren.results.csv; --permute adds Empirical_p from shuffles of the values within "
                   "the strata; at most 1024 strata (single process; scoary_amd extension)")
    a.add_argument("--quantitative-fwer", dest="quantitative_fwer", action="store_true", default=False,
                   help="With --quantitative and --permute X (X >= 10): add the column Westfall_Young_p to the rank-sum "
                   "results -- and, with --quantitative-strata, to the van Elteren results -- the single-step maxT "
                   "family-wise p over all genes of the table, from the same permutations that give Empirical_p "
                   "(single process; scoary_amd extension)")
    a.add_argument("--quantitative-fwer-stepdown", dest="quantitative_fwer_stepdown", action="store_true",
                   default=False,
                   help="With --quantitative and --permute X (X >= 10): add the column Westfall_Young_stepdown_p to the "
                   "rank-sum results -- and, with --quantitative-strata, to the van Elteren results -- the step-down "
                   "maxT family-wise p: a gene is compared with the genes at its rank and behind, so the p is never "
                   "above Westfall_Young_p (single process; scoary_amd extension)")
    a.add_argument("--quantitative-shift", dest="quantitative_shift", action="store_true", default=False,
                   help="With --quantitative: add the columns Rank_sum_shift, Rank_sum_shift_lower and "
                   "Rank_sum_shift_upper to the rank-sum results -- the Hodges-Lehmann estimate of the shift of the "
                   "trait with the gene (the median of all differences isolate with the gene minus isolate without, "
                   "in the trait's units) and its distribution-free confidence limits; R's wilcox.test(conf.int = "
                   "TRUE); needs no permutations (single process; scoary_amd extension)")
    a.add_argument("--quantitative-shift-level", dest="quantitative_shift_level", type=float, default=None,
                   metavar="FLOAT",
                   help="With --quantitative-shift: the confidence level of the limits, inside (0, 1) (default 0.95)")
    a.add_argument("--no_pairwise", action="store_true", default=False,
                   help="Population-structure-naive analysis only (Fisher's test, odds ratios)")
    a.add_argument("--collapse", action="store_true", default=False,
                   help="Merge genes with identical distribution patterns into one unit")
    a.add_argument("--seed", type=int, default=DEFAULT_SEED,
                   help="Seed of the counter-based permutation generator (scoary_amd extension)")
    m = ap.add_argument_group("Misc options")
    m.add_argument("--threads", type=int, default=1,
                   help="Accepted for compatibility; the GPU path does not use host threads")
    m.add_argument("--test", action="store_true", default=False,
                   help="Run on the bundled example data (needs the path in SCOARY_EXAMPLEDATA)")
    m.add_argument("--citation", action="store_true", default=False,
                   help="Show citation information and exit")
    m.add_argument("--version", action="version", version=SCOARY_COMPAT_VERSION)
    args = ap.parse_args(argv)
    if len(args.p_value_cutoff) == 1:
        cutoffs = {c: args.p_value_cutoff[0] for c in args.correction}
    else:
        cutoffs = dict(zip(args.correction, args.p_value_cutoff))
    return args, cutoffs


CITATION = ("If you use Scoary, please cite: Brynildsrud O, Bohlin J, Scheffer L, Eldholm V. "
            "Rapid scoring of genes in microbial pan-genome-wide association studies with "
            "Scoary. Genome Biol. 2016;17:238.  (scoary_amd re-implements Scoary's Fisher / "
            "permutation path for AMD MI355X.)")


def main(**kwargs):
    """The command-line flow of methods.py:49-330 for the association path."""
    if len(kwargs) == 0:
        args, cutoffs = ScoaryArgumentParser()
    else:
        args, cutoffs = kwargs["args"], kwargs["cutoffs"]
        if "statusbar" in kwargs:
            sys.stdout = kwargs["statusbar"]
    if args.citation:
        sys.exit(CITATION)
    if args.test:
        ex = os.environ.get("SCOARY_EXAMPLEDATA")
        if not ex:
            sys.exit("--test needs SCOARY_EXAMPLEDATA=<dir with Gene_presence_absence.csv and "
                     "Tetracycline_resistance.csv>")
        args.correction, args.delimiter, args.grabcols = ["I", "EPW"], ",", []
        args.genes = os.path.join(ex, "Gene_presence_absence.csv")
        args.traits = os.path.join(ex, "Tetracycline_resistance.csv")
        args.max_hits = args.newicktree = args.restrict_to = None
        args.no_pairwise, args.outdir, args.permute = False, "./", 0
        args.p_value_cutoff, args.start_col, args.threads = [0.05, 0.05], 15, 4
        args.upgma_tree, args.write_reduced, args.no_time, args.collapse = True, False, False, False
        cutoffs = {"I": 0.05, "EPW": 0.05}

    from . import dist
    world, rank, _local = dist.init_from_env()
    start = _time.time()
    stamp = "" if args.no_time else _time.strftime("_%d_%m_%Y_%H%M")
    if not args.outdir.endswith("/"):
        args.outdir += "/"
    os.makedirs(args.outdir, exist_ok=True)
    console = logging.StreamHandler(sys.stdout)
    console.setFormatter(logging.Formatter("%(message)s"))
    console.setLevel(logging.INFO)
    logfile = logging.FileHandler(os.path.join(
        args.outdir, "scoary%s%s.log" % (stamp, "" if rank == 0 else ".rank%d" % rank)), mode="w")
    logfile.setFormatter(logging.Formatter("%(asctime)s    %(message)s", "%m/%d/%Y %I:%M:%S %p"))
    log.addHandler(console)
    log.addHandler(logfile)
    counts = _LevelCounter()
    log.addHandler(counts)
    log.info("==== Scoary started ====")
    log.info("Command: " + " ".join(sys.argv))
    starter = None
    try:
        _validate(args, cutoffs)
        seed = getattr(args, "seed", DEFAULT_SEED)
        allowed = None
        if args.restrict_to is not None:
            with open(args.restrict_to, "r") as f:
                allowed = {iso: "all" for line in f for iso in line.rstrip().split(",")}
        elif args.write_reduced:
            sys.exit("You cannot use the -w argument without specifying a subset (-r)")
        _stage.reset()
        # The first GPU call of the process -- torch import, library load, HIP context, warm-up: about a
        # second -- and the read of the gene table need nothing from each other, and the native reader
        # runs outside the interpreter lock: a single process starts the engine on a helper thread and
        # joins it after the read (a 2.5 GB table reads in 0.6 s: the second shrinks to what the read
        # does not cover).  Under torchrun the process group already imported torch and picked the device.
        if world == 1 and not dist._initialized_safe() and os.environ.get("SCOARY_OVERLAP_STARTUP", "1") == "1":
            import threading
            started = {}

            def _start_engine():
                t0 = _time.perf_counter()
                try:
                    get_engine()
                except BaseException as e:          # re-raised on the main thread at the join
                    started["error"] = e
                started["seconds"] = _time.perf_counter() - t0
            starter = threading.Thread(target=_start_engine, name="scoary-engine-start", daemon=True)
            starter.start()
        else:
            with _stage("import torch, HIP library, engine"):
                get_engine()
        with open(args.genes, "r", newline=None) as genes, \
                open(args.traits, "r", newline=None) as traits:
            log.info("Reading gene presence absence file")
            grab = [-999] if args.grabcols == "ALL" else args.grabcols
            with _stage("read gene table"):
                gd = Csv_to_dic_Roary(genes, args.delimiter, grab, startcol=int(args.start_col) - 1,
                                      allowed_isolates=allowed, writereducedset=args.write_reduced,
                                      time=stamp, outdir=args.outdir)
            if starter is not None:
                with _stage("engine start not covered by the read"):
                    starter.join()
                _stage.seconds["import torch, HIP library, engine (helper thread, under the read)"] = \
                    started.get("seconds", 0.0)
                if "error" in started:
                    raise started["error"]
            genedic, strains = gd["Roarydic"], gd["Strains"]
            upgmatree = None
            if args.newicktree is None and not args.no_pairwise:
                log.info("Creating Hamming distance matrix based on gene presence/absence")
                from . import tree as T
                log.info("Building UPGMA tree from distance matrix")
                upgmatree = T.upgma(get_engine(), gd["Zero_ones_matrix"].file_rows(), strains)
                _preload_scipy()
            elif args.no_pairwise:
                log.info("Ignoring relatedness among input sample and performing only "
                         "population structure-naive analysis.")
            else:
                log.info("Reading custom tree file")
                from . import tree as T
                upgmatree, members = T.read_newick(args.newicktree)
                if sorted(strains) != sorted(members):
                    if args.restrict_to is None:
                        sys.exit("CRITICAL: Please make sure that isolates in your custom tree "
                                 "match those in your gene presence absence file.")
                    if not all(i in members for i in strains):
                        sys.exit("CRITICAL: Your provided tree file did not contain all the "
                                 "isolates in your gene presence absence file.")
                    log.info("Pruning phylogenetic tree to correspond to set of included isolates")
                    keepset = set(strains)
                    upgmatree = T.prune_missing(upgmatree, [i for i in members if i not in keepset])
            log.info("Reading traits file")
            with _stage("read traits"):
                traitsdic, prunedic = Csv_to_dic(traits, args.delimiter, allowed, strains)
        t_loaded = _time.time()
        log.info("Finished loading files into memory.\n\n")
        log.info("==== Performing statistics ====")
        for line in filtrationoptions(cutoffs, args.collapse):
            log.info(line)
        log.info("Tallying genes and performing statistical analyses")
        # --no_pairwise: Fisher-statistic permutations for every gene (north_star);
        # default mode: tree-statistic permutations of the surviving genes, done
        # in the pairwise stage like the reference does.
        strata = None
        if getattr(args, "permute_strata", None) or getattr(args, "cmh", None):
            # the authoritative call, on the strains the reader kept (_validate's early one reads the header on its
            # own: should the two ever disagree, the same exit message appears here, after the engine has started)
            strata, labels = strata_indices(args.strata_map, strains)
            sizes = np.bincount(strata, minlength=len(labels))
            if getattr(args, "cmh", None):
                log.info("Cochran-Mantel-Haenszel test over %d strata of %d to %d isolates (%s)"
                         % (len(labels), int(sizes.min()), int(sizes.max()), args.cmh))
            if args.permute >= 10:
                log.info("Permuting trait labels within %d strata of %d to %d isolates (%s)"
                         % (len(labels), int(sizes.min()), int(sizes.max()), args.permute_strata or args.cmh))
        # the flags' keywords, by _validate's mapping; the two flags that name a file arrive as ``strata`` and a bool
        flags = {rule.kw: getattr(args, rule.flag[2:].replace("-", "_"), False)
                 for rule in ALL_RULES if rule.flag not in ("--cmh", "--permute-strata")}
        res = Setup_results(genedic, traitsdic, args.collapse,
                            permutations=args.permute if args.no_pairwise else 0, seed=seed,
                            early_abort=getattr(args, "permute_early_abort", False), strata=strata,
                            cmh=bool(getattr(args, "cmh", None)),
                            cmh_exact_level=getattr(args, "cmh_exact_level", None) or DEFAULT_EXACT_LEVEL, **flags)
        t_stats = _time.time()
        if args.upgma_tree and rank == 0:
            # (with --no_pairwise there is no tree and the reference writes str(None) + ";", :277-280, :741-751)
            StoreUPGMAtreeToFile(upgmatree, args.outdir, time=stamp)
        if rank == 0:           # every rank holds the gathered results; one writes
            StoreResults(res["Results"], args.max_hits, cutoffs, upgmatree,
                         res["Gene_trait_combinations"], prunedic, args.outdir, args.permute,
                         args.threads, args.no_pairwise, genedic, gd["Extracols"],
                         gd["Firstcolnames"], time=stamp, delimiter=args.delimiter, seed=seed)
        if getattr(args, "quantitative", None) and rank == 0:
            names, values = read_quantitative_file(args.quantitative, args.delimiter, strains)
            qfwer = bool(getattr(args, "quantitative_fwer", False))
            qsd = bool(getattr(args, "quantitative_fwer_stepdown", False))
            qshift = bool(getattr(args, "quantitative_shift", False))
            for text in _rank_shift_refusals(qshift, True, None, values):
                sys.exit(text)
            with _stage("rank-sum test of the quantitative traits"):
                StoreRanksumResults(Ranksum_results(genedic, names, values, permutations=args.permute, seed=seed,
                                                    fwer=qfwer, stepdown=qsd, shift=qshift,
                                                    shift_level=_shift_level(args)),
                                    genedic, args.max_hits, args.outdir, time=stamp, delimiter=args.delimiter)
            if getattr(args, "quantitative_strata", None):
                qstrata = strata_indices(args.quantitative_strata_map, strains)[0]
                with _stage("van Elteren test of the quantitative traits"):
                    StoreVanElterenResults(VanElteren_results(genedic, names, values, qstrata,
                                                              permutations=args.permute, seed=seed,
                                                              fwer=qfwer, stepdown=qsd),
                                           genedic, args.max_hits, args.outdir, time=stamp, delimiter=args.delimiter)
        if getattr(args, "categorical", None) and rank == 0:
            names, labels = read_categorical_file(args.categorical, args.delimiter, strains)
            cfwer = bool(getattr(args, "categorical_fwer", False))
            csd = bool(getattr(args, "categorical_fwer_stepdown", False))
            with _stage("chi-square test of the categorical traits"):
                StoreCategoricalResults(Categorical_results(genedic, names, labels, permutations=args.permute,
                                                            seed=seed, exits=True, fwer=cfwer, stepdown=csd),
                                        genedic, args.max_hits, args.outdir, time=stamp, delimiter=args.delimiter,
                                        stepdown=csd)
            if getattr(args, "categorical_strata", None):
                cstrata = strata_indices(args.categorical_strata_map, strains)[0]
                with _stage("generalized CMH test of the categorical traits"):
                    StoreGcmhResults(Gcmh_results(genedic, names, labels, cstrata, permutations=args.permute,
                                                  seed=seed, fwer=cfwer, stepdown=csd),
                                     genedic, args.max_hits, args.outdir, time=stamp, delimiter=args.delimiter,
                                     stepdown=csd)
        if getattr(args, "covariates", None) and rank == 0:
            cnames, covariates = read_covariates_file(args.covariates, args.delimiter, strains)
            for text in _score_refusals(True, False, cnames, covariates, source=args.covariates, exits=True):
                sys.exit(text)
            names, values = binary_trait_values(traitsdic, strains)
            with _stage("logistic score test of the traits"):
                StoreScoreResults(Score_results(genedic, names, values, cnames, covariates, kind="logistic",
                                                spa=getattr(args, "covariates_spa", False),
                                                spa_cutoff=getattr(args, "covariates_spa_cutoff", None)),
                                  genedic, args.max_hits, args.outdir, time=stamp, delimiter=args.delimiter)
            if getattr(args, "quantitative", None):
                names, values = read_quantitative_file(args.quantitative, args.delimiter, strains)
                with _stage("linear score test of the quantitative traits"):
                    StoreScoreResults(Score_results(genedic, names, values, cnames, covariates, kind="linear"),
                                      genedic, args.max_hits, args.outdir, time=stamp, delimiter=args.delimiter)
        log.info("Stage seconds: load (+tree) %.2f, association (+permutations) %.2f, pairwise stage and "
                 "output %.2f" % (t_loaded - start, t_stats - t_loaded, _time.time() - t_stats))
        gene_bytes = os.path.getsize(args.genes) if os.path.isfile(args.genes) else 0
        log.info("Stage detail: " + "; ".join("%s %.3f s" % kv for kv in _stage.seconds.items())
                 + ("; gene table %.0f MB" % (gene_bytes / 1e6) if gene_bytes else ""))
        log.info("\n")
        log.info("==== Finished ====")
        log.info("Checked a total of %d genes for associations to %d trait(s). Total time "
                 "used: %d seconds." % (len(genedic), len(traitsdic), int(_time.time() - start)))
    except SystemExit as e:
        if starter is not None:
            starter.join(120)          # never tear the interpreter down under a thread that is inside HIP start-up
        log.exception("CRITICAL:")
        for hnd in (logfile, console, counts):
            log.removeHandler(hnd)
        dist.shutdown()
        sys.exit(e.code)
    except BaseException:
        if starter is not None:
            starter.join(120)
        raise
    if counts.n.get("CRITICAL", 0):
        log.info("Scoary finished successfully, but with CRITICAL ERRORS. Please check your log file.")
    elif counts.n.get("ERROR", 0):
        log.info("Scoary finished successfully, but with ERRORS. Please check your log file.")
    elif counts.n.get("WARNING", 0):
        log.info("Scoary finished successfully, but with WARNINGS. Please check your log file.")
    else:
        log.info("No warnings were recorded.")
    for hnd in (logfile, console, counts):
        log.removeHandler(hnd)
    logfile.close()
    dist.shutdown()
    sys.exit(0)


# ---------------------------------------------------------------------------
# --quantitative FILE: the rank-sum test of measured traits (spec S15).  A stage and result files of its own: a
# measured trait has no 2 x 2 table and no Fisher p, so nothing of it enters the per-trait results file or the
# tables of its optional columns.
# ---------------------------------------------------------------------------
RANKSUM_COLUMNS = ("Number_with_gene", "Number_without_gene", "Rank_sum_AUC", "Rank_sum_p", "Bonferroni_p",
                   "Benjamini_H_p")
# a refusal as the command line reports it / as Ranksum_results raises it
RANKSUM_TEXT = {
    "no_pairwise": ("Cannot use --quantitative without --no_pairwise. The rank-sum test is a population "
                    "structure-naive test of every gene",
                    "quantitative traits need no_pairwise: the rank-sum test is population structure-naive"),
    "collapse": ("Cannot use --quantitative together with --collapse. The rank-sum test is a test of every gene of "
                 "the table", "quantitative traits exclude collapse"),
    "strata": ("Cannot use --quantitative together with --permute-strata. The values are shuffled over all isolates "
               "with a value; a shuffle within strata is not implemented",
               "quantitative traits exclude strata: their values are shuffled over all valid isolates"),
    "ranks": ("Cannot use --quantitative under more than one rank: the test runs over all genes in a single process",
              "quantitative traits need a single process"),
}


def _ranksum_refusals(no_pairwise, collapse, strata, exits=False):
    """The messages of the --quantitative rules that a run breaks, in the order they are reported (``exits``: as the
    command line's exit messages, else as Ranksum_results' ValueErrors)."""
    if not no_pairwise:
        yield RANKSUM_TEXT["no_pairwise"][not exits]
    if collapse:
        yield RANKSUM_TEXT["collapse"][not exits]
    if strata:
        yield RANKSUM_TEXT["strata"][not exits]
    from . import dist
    if dist.world_rank()[0] > 1:
        yield RANKSUM_TEXT["ranks"][not exits]


def _read_side_traits(path, delimiter, strains, what, cell, empty):
    """The trait file of a side stage (``what``: "quantitative" or "categorical"): a header row (its first cell is
    ignored, the others name the traits), then one row per isolate: its name and one cell per trait.  Returns
    (names, ``empty(T, N)`` over ``strains`` with ``cell(text, path, isolate, trait, line)`` -- which parses or
    refuses -- in the place of every cell that is none of MISSING_TRAIT): isolates the analysis does not hold are
    ignored, isolates of ``strains`` the file does not name are missing in every trait."""
    with open(path, "r", newline=None) as f:
        rows = [r for r in csv.reader(f, delimiter=delimiter) if r]
    if not rows or len(rows[0]) < 2:
        sys.exit("Please check that the %s traits file %s is formatted properly and contains at least one "
                 "trait" % (what, path))
    names = list(rows[0][1:])
    if len(set(names)) != len(names):
        sys.exit("The %s traits file %s names a trait more than once" % (what, path))
    col = {s: j for j, s in enumerate(strains)}
    out = empty(len(names), len(strains))
    seen = set()
    for line, row in enumerate(rows[1:], start=2):
        iso = row[0]
        if iso in seen:
            sys.exit("The %s traits file %s names isolate %s more than once (line %d)" % (what, path, iso, line))
        seen.add(iso)
        if len(row) != len(names) + 1:
            sys.exit("The %s traits file %s has %d cells in line %d, its header has %d"
                     % (what, path, len(row), line, len(names) + 1))
        if iso not in col:
            continue
        for t, text in enumerate(row[1:]):
            if text not in MISSING_TRAIT:
                out[t][col[iso]] = cell(text, path, iso, names[t], line)
    return names, out


def read_quantitative_file(path, delimiter, strains):
    """--quantitative FILE: a header row (its first cell is ignored, the others name the traits), then one row per
    isolate: its name and one cell per trait, a number (float()) or one of MISSING_TRAIT.  Returns (names, float64
    [T, N] over ``strains`` with nan = missing): isolates the analysis does not hold are ignored, isolates of
    ``strains`` the file does not name are missing in every trait."""
    def number(text, path, iso, trait, line):
        try:
            x = float(text)
        except ValueError:
            x = np.nan
        if not np.isfinite(x):
            sys.exit("The quantitative traits file %s has the cell %r for isolate %s, trait %s (line %d): a cell "
                     "is a finite number or one of %s" % (path, text, iso, trait, line,
                                                          ",".join(repr(m) for m in MISSING_TRAIT)))
        return x
    return _read_side_traits(path, delimiter, strains, "quantitative", number,
                             lambda T, N: np.full((T, N), np.nan, dtype=np.float64))


def _side_stage_limits(what, eng, N, strata=None):
    """The ValueErrors the side stages share (``what``: "quantitative" or "categorical"): more isolates than the
    generators take and, for a stratified stage, strata that are not N stratum indices or too many."""
    if strata is not None and (strata.shape != (N,) or not np.issubdtype(strata.dtype, np.integer)
                               or strata.min() < 0):
        raise ValueError("%s traits: strata must be %d stratum indices, one per isolate" % (what, N))
    if N > eng.ranksum_max_isolates():
        raise ValueError("%s traits take at most %d isolates; this analysis has %d"
                         % (what, eng.ranksum_max_isolates(), N))
    from . import _abi
    if strata is not None and int(strata.max()) + 1 > _abi.PERM_MAX_STRATA:
        raise ValueError("%s traits take at most %d strata; these are %d"
                         % (what, _abi.PERM_MAX_STRATA, int(strata.max()) + 1))


def Ranksum_results(genedic, names, values, permutations=0, seed=DEFAULT_SEED, no_pairwise=True, collapse=False,
                    strata=None, fwer=False, stepdown=False, shift=False, shift_level=0.95):
    """The rank-sum stage (spec S15) of the traits ``names`` with the values float64 [T, N] (nan = missing) over the
    isolates of ``genedic``: {name: dict(n, tie_groups, m, auc, p, testable [G]; r [G] with permutations >= 10;
    r_fwer [G] with ``fwer``, spec S17; r_sd [G] with ``stepdown``, spec S18; shift, shift_lower, shift_upper [G] with
    ``shift``, the Hodges-Lehmann shift and its limits at ``shift_level``, spec S19)}, arrays in the gene table's
    order.  Raises ValueError where the command line refuses --quantitative, --quantitative-fwer,
    --quantitative-fwer-stepdown or --quantitative-shift."""
    for text in _ranksum_refusals(no_pairwise, collapse, strata is not None):
        raise ValueError(text)
    for text in _rank_wy_refusals(fwer, True, permutations):
        raise ValueError(text)
    for text in _rank_sd_refusals(stepdown, True, permutations):
        raise ValueError(text)
    for text in _rank_shift_refusals(shift, True, shift_level if shift else None, values):
        raise ValueError(text)
    table = _as_table(genedic)
    eng = get_engine()
    values = np.asarray(values, dtype=np.float64)
    if values.ndim != 2 or values.shape != (len(names), len(table.strains)):
        raise ValueError("quantitative traits: values must be [%d traits, %d isolates]"
                         % (len(names), len(table.strains)))
    _side_stage_limits("quantitative", eng, values.shape[1])
    genes = table.on_device(eng)
    plan = eng.ranksum_plan(values)
    res = eng.ranksum(genes, plan)
    permutations = int(permutations)
    r = r_fwer = r_sd = None
    if stepdown:                 # the step-down run gives all three counts; the single-step one costs nothing extra
        r, r_fwer, r_sd = (x.cpu().numpy() for x in eng.ranksum_stepdown(genes, plan, res, permutations, seed)[:3])
        r_fwer = r_fwer if fwer else None
    elif fwer:                   # one pass over the permutations gives both counts
        r, r_fwer = (x.cpu().numpy() for x in eng.ranksum_westfall_young(genes, plan, res, permutations, seed)[:2])
    elif permutations >= 10:
        r = eng.ranksum_permute(genes, plan, res["d"], permutations, seed).cpu().numpy()
    hl = None
    if shift:
        hl = {k: v.cpu().numpy() for k, v in eng.ranksum_shift(genes, plan, res, level=shift_level).items()}
    m, auc, p = (res[k].cpu().numpy() for k in ("m", "auc", "p"))
    out = {}
    for t, name in enumerate(names):
        n = int(plan.n[t])
        f_positive = n >= 2 and float(n + 1) - float(plan.tiesum_host[t]) / (float(n) * float(n - 1)) > 0
        testable = (m[t] > 0) & (m[t] < n) & bool(f_positive)
        out[name] = dict(n=n, tie_groups=int(plan.tie_groups[t]), m=m[t], auc=auc[t], p=p[t], testable=testable)
        if r is not None:
            out[name]["r"] = r[t]
            out[name]["permutations"] = permutations
        if r_fwer is not None:
            out[name]["r_fwer"] = r_fwer[t]
        if r_sd is not None:
            out[name]["r_sd"] = r_sd[t]
        if hl is not None:
            out[name].update(shift=hl["shift"][t], shift_lower=hl["lower"][t], shift_upper=hl["upper"][t])
        log.info("Rank-sum test of %s: %d isolates with a value, %d tie groups, %d genes tested"
                 % (name, n, out[name]["tie_groups"], int(testable.sum())))
    return out


# the columns of a side stage's permutation counts and their keys: (count + 1) / (permutations + 1), only next to r
PERMUTATION_COLUMNS = (("Empirical_p", "r"), ("Westfall_Young_p", "r_fwer"), ("Westfall_Young_stepdown_p", "r_sd"))


def _store_side_results(results, genedic, max_hits, outdir, time, delimiter, test_columns, cells, suffix, what,
                        rank=False, stepdown=False, last=None):
    """The result files of a side stage (the four Store*Results below): per trait the testable genes in ascending p
    (ties in file order), Bonferroni and Benjamini-Hochberg over them, every cell double-quoted.  ``test_columns``
    name the stage's fixed columns: the two carrier counts, the test's own -- their cells are ``cells(res, g)`` --
    and the two adjusted p.  Behind them come the columns a result carries the keys for: with ``rank`` the shift and
    its limits, then Empirical_p, Westfall_Young_p and, with ``rank`` or ``stepdown``, Westfall_Young_stepdown_p (the
    categorical stages ask for it with ``stepdown``: a result that merely carries r_sd gets no column there).  Behind
    all of them ``last(res, idx)`` -> (column names, one list of cells per gene of ``idx``), where a stage gives it."""
    table = _as_table(genedic)
    files = []
    for name, res in results.items():
        with_shift = rank and all(key in res for _column, key in RANK_SHIFT_COLUMNS)
        counts = [(column, key) for column, key in PERMUTATION_COLUMNS[:3 if rank or stepdown else 2]
                  if "r" in res and key in res]
        columns = ROARY_HEAD + list(test_columns) + \
            ([column for column, _key in RANK_SHIFT_COLUMNS] if with_shift else []) + [column for column, _key in counts]
        idx = np.flatnonzero(res["testable"])
        last_columns, last_cells = last(res, idx) if last else ([], [])
        columns += list(last_columns)
        fname = outdir + name + time + suffix
        with open(fname, "w") as out:
            out.write(delimiter.join('"' + c + '"' for c in columns) + "\n")
            if len(idx):
                p = res["p"][idx]
                order = np.argsort(p, kind="stable")
                bonf, bh = bonferroni_bh(p, len(idx), order=order)
                shown = len(idx) if max_hits is None else max(0, min(max_hits, len(idx)))
                for k in order[:shown]:
                    g = int(idx[k])
                    gene = table.ids[g]
                    row = gene.split("_|_") if "_|_" in gene else [gene, str(table.nugn[g]),
                                                                   str(table.annotation[g])]
                    m = int(res["m"][g])
                    row += [_fmt(m), _fmt(res["n"] - m)] + cells(res, g) + [_fmt(bonf[k]), _fmt(bh[k])]
                    if with_shift:           # an infinite limit is _fmt's "inf" / "-inf", as in the odds ratio's limits
                        row += [_fmt(res[key][g]) for _column, key in RANK_SHIFT_COLUMNS]
                    row += [_fmt((int(res[key][g]) + 1.0) / (res["permutations"] + 1.0)) for _column, key in counts]
                    if last_columns:
                        row += last_cells[k]
                    out.write(delimiter.join('"' + c + '"' for c in row) + "\n")
        log.info("Storing %s results: %s" % (what, fname))
        files.append(fname)
    return files


def _rank_cells(res, g):
    return [_fmt(res["auc"][g]), _fmt(res["p"][g])]


def StoreRanksumResults(results, genedic, max_hits, outdir, time="", delimiter=","):
    """Write ``<outdir><trait><time>.ranksum.results.csv`` for every trait of Ranksum_results: the testable genes in
    ascending Rank_sum_p (ties in file order), Bonferroni and Benjamini-Hochberg over them, every cell
    double-quoted.  Returns the file names."""
    return _store_side_results(results, genedic, max_hits, outdir, time, delimiter, RANKSUM_COLUMNS, _rank_cells,
                               ".ranksum.results.csv", "rank-sum", rank=True)


# ---------------------------------------------------------------------------
# --categorical FILE: the gene x K-class chi-square test of labelled traits (spec S20).  A stage and result files of
# its own, as --quantitative has them: a label of more than two levels has no 2 x 2 table and no Fisher p.
# ---------------------------------------------------------------------------
CATEGORICAL_COLUMNS = ("Number_with_gene", "Number_without_gene", "Carriers_by_class", "Most_enriched_class", "Chi2",
                       "Chi2_df", "Cramers_V", "Chi2_p", "Bonferroni_p", "Benjamini_H_p")
# a refusal as the command line reports it / as Categorical_results raises it
CATEGORICAL_TEXT = {
    "no_pairwise": ("Cannot use --categorical without --no_pairwise. The chi-square test is a population "
                    "structure-naive test of every gene",
                    "categorical traits need no_pairwise: the chi-square test is population structure-naive"),
    "collapse": ("Cannot use --categorical together with --collapse. The chi-square test is a test of every gene of "
                 "the table", "categorical traits exclude collapse"),
    "strata": ("Cannot use --categorical together with --permute-strata. The labels are shuffled over all isolates "
               "with a label; a shuffle within strata is not implemented",
               "categorical traits exclude strata: their labels are shuffled over all valid isolates"),
    "ranks": ("Cannot use --categorical under more than one rank: the test runs over all genes in a single process",
              "categorical traits need a single process"),
    "classes": ("Cannot use --categorical with the trait %s: it has %d classes among the analysed isolates, the test "
                "takes at most %d. Merge rare classes into one before the run",
                "categorical trait %s has %d classes, at most %d are taken: merge rare classes"),
}


def categorical_classes(labels):
    """The classes of one trait's labels (a string per isolate, None = missing): sorted as Python strings."""
    return sorted(set(x for x in labels if x is not None))


def _class_codes(labels, N):
    """(classes, codes) of the labels [T][N]: every trait's classes (categorical_classes) and its isolates' class
    numbers, 1 .. K in that order and 0 = missing, int16 [T, N]."""
    classes = [categorical_classes(row) for row in labels]
    codes = np.zeros((len(labels), N), dtype=np.int16)
    for t, row in enumerate(labels):
        number = {c: k + 1 for k, c in enumerate(classes[t])}
        codes[t] = [number[x] if x is not None else 0 for x in row]
    return classes, codes


def _categorical_refusals(no_pairwise, collapse, strata, names=(), labels=(), exits=False):
    """The messages of the --categorical rules that a run breaks, in the order they are reported (``exits``: as the
    command line's exit messages, else as Categorical_results' ValueErrors).  ``names``, ``labels``: the traits, once
    they are read."""
    from . import _abi, dist
    if not no_pairwise:
        yield CATEGORICAL_TEXT["no_pairwise"][not exits]
    if collapse:
        yield CATEGORICAL_TEXT["collapse"][not exits]
    if strata:
        yield CATEGORICAL_TEXT["strata"][not exits]
    if dist.world_rank()[0] > 1:
        yield CATEGORICAL_TEXT["ranks"][not exits]
    for name, row in zip(names, labels):
        k = len(categorical_classes(row))
        if k > _abi.CATEGORICAL_MAX_CLASSES:
            yield CATEGORICAL_TEXT["classes"][not exits] % (name, k, _abi.CATEGORICAL_MAX_CLASSES)


def read_categorical_file(path, delimiter, strains):
    """--categorical FILE: a header row (its first cell is ignored, the others name the traits), then one row per
    isolate: its name and one cell per trait, any string as the label or one of MISSING_TRAIT.  Returns (names,
    labels [T][N] over ``strains``, None = missing): isolates the analysis does not hold are ignored, isolates of
    ``strains`` the file does not name are missing in every trait."""
    return _read_side_traits(path, delimiter, strains, "categorical", lambda text, *_where: text,
                             lambda T, N: [[None] * N for _ in range(T)])


def Categorical_results(genedic, names, labels, permutations=0, seed=DEFAULT_SEED, no_pairwise=True, collapse=False,
                        strata=None, exits=False, fwer=False, stepdown=False):
    """The chi-square stage (spec S20) of the traits ``names`` with the labels [T][N] (a string per isolate, None =
    missing) over the isolates of ``genedic``: {name: dict(classes, n, nk [K], df, a [G, K], m, x2, v, p, testable
    [G]; r [G] and permutations with permutations >= 10; r_fwer [G] with ``fwer``, spec S22; r_sd [G] with
    ``stepdown``, spec S23)}, arrays in the gene table's order.  Raises ValueError where the command line refuses
    --categorical, --categorical-fwer or --categorical-fwer-stepdown (``exits``: exits with the command line's message
    instead)."""
    for text in _categorical_refusals(no_pairwise, collapse, strata is not None, names, labels, exits=exits):
        if exits:
            sys.exit(text)
        raise ValueError(text)
    for text in _cat_wy_refusals(fwer, True, permutations):
        if exits:
            sys.exit(text)
        raise ValueError(text)
    for text in _cat_sd_refusals(stepdown, True, permutations):
        if exits:
            sys.exit(text)
        raise ValueError(text)
    table = _as_table(genedic)
    eng = get_engine()
    N = len(table.strains)
    if len(labels) != len(names) or any(len(row) != N for row in labels):
        raise ValueError("categorical traits: labels must be [%d traits, %d isolates]" % (len(names), N))
    _side_stage_limits("categorical", eng, N)
    classes, codes = _class_codes(labels, N)
    genes = table.on_device(eng)
    plan = eng.categorical_plan(codes)
    res = eng.categorical(genes, plan)
    permutations = int(permutations)
    r = r_fwer = r_sd = None
    if stepdown:                 # the step-down run gives all three counts; the single-step one costs nothing extra
        r, r_fwer, r_sd = (x.cpu().numpy() for x in eng.categorical_stepdown(genes, plan, res, permutations, seed)[:3])
        r_fwer = r_fwer if fwer else None
    elif fwer:
        r, r_fwer = (x.cpu().numpy() for x in eng.categorical_westfall_young(genes, plan, res, permutations, seed)[:2])
    elif permutations >= 10:
        r = eng.categorical_permute(genes, plan, res["a"], permutations, seed).cpu().numpy()
    a, m, x2, p, v = (res[k].cpu().numpy() for k in ("a", "m", "x2", "p", "v"))
    out = {}
    for t, name in enumerate(names):
        n, K = int(plan.n[t]), len(classes[t])
        testable = (m[t] > 0) & (m[t] < n) & bool(n >= 2 and int(plan.classes[t]) >= 2)
        out[name] = dict(classes=classes[t], n=n, nk=plan.nk_host[t, :K].copy(), df=int(plan.classes[t]) - 1,
                         a=a[t][:, :K], m=m[t], x2=x2[t], v=v[t], p=p[t], testable=testable)
        if r is not None:
            out[name]["r"] = r[t]
            out[name]["permutations"] = permutations
        if r_fwer is not None:
            out[name]["r_fwer"] = r_fwer[t]
        if r_sd is not None:
            out[name]["r_sd"] = r_sd[t]
        log.info("Chi-square test of %s: %d isolates with a label in %d classes, %d genes tested"
                 % (name, n, K, int(testable.sum())))
    return out


def most_enriched_class(a, nk):
    """The index of the class with the largest a_k / n_k among the non-empty ones, compared as a_k n_j against
    a_j n_k in integers; ties go to the first class."""
    best = None
    for k, (ak, n) in enumerate(zip(a, nk)):
        if n > 0 and (best is None or int(ak) * int(nk[best]) > int(a[best]) * int(n)):
            best = k
    return best


def StoreCategoricalResults(results, genedic, max_hits, outdir, time="", delimiter=",", stepdown=False):
    """Write ``<outdir><trait><time>.categorical.results.csv`` for every trait of Categorical_results: the testable
    genes in ascending Chi2_p (ties in file order), Bonferroni and Benjamini-Hochberg over them, every cell
    double-quoted.  ``stepdown`` (--categorical-fwer-stepdown): Westfall_Young_stepdown_p from the results' r_sd, the
    last column.  Returns the file names."""
    def cells(res, g):
        a = res["a"][g]
        return ["|".join("%s=%d" % (c, int(x)) for c, x in zip(res["classes"], a)),
                res["classes"][most_enriched_class(a, res["nk"])], _fmt(res["x2"][g]), _fmt(res["df"]),
                _fmt(res["v"][g]), _fmt(res["p"][g])]
    return _store_side_results(results, genedic, max_hits, outdir, time, delimiter, CATEGORICAL_COLUMNS, cells,
                               ".categorical.results.csv", "chi-square", stepdown=stepdown)


# ---------------------------------------------------------------------------
# --categorical-strata FILE: the generalized Cochran-Mantel-Haenszel test of the labelled traits over strata (spec
# S21), next to the chi-square stage: result files of its own, and nothing of the chi-square files changes.
# ---------------------------------------------------------------------------
GCMH_COLUMNS = ("Number_with_gene", "Number_without_gene", "Carriers_by_class", "Expected_by_class",
                "Most_enriched_class", "GCMH", "GCMH_df", "GCMH_p", "Bonferroni_p", "Benjamini_H_p")
GCMH_TEXT = {
    "categorical": "Cannot use --categorical-strata without --categorical. Its strata are those of the generalized "
                   "Cochran-Mantel-Haenszel test of the categorical traits",
    "file": "Could not find the strata file of --categorical-strata: %s",
    "strata": "The strata file %s names %d strata for the analysed isolates; --categorical-strata takes at most %d",
}


def Gcmh_results(genedic, names, labels, strata, permutations=0, seed=DEFAULT_SEED, no_pairwise=True, collapse=False,
                 fwer=False, stepdown=False):
    """The generalized CMH stage (spec S21) of the traits ``names`` with the labels [T][N] (a string per isolate, None
    = missing) and the stratum index of every isolate ``strata`` (N integers) over the isolates of ``genedic``: {name:
    dict(classes, n, strata (those with a labelled isolate), a [G, K], e [G, K], m, q, df, p, testable [G]; r [G] and
    permutations with permutations >= 10; r_fwer [G] with ``fwer``, spec S22; r_sd [G] with ``stepdown``, spec S23)},
    arrays in the gene table's order.  Raises ValueError where the command line refuses --categorical,
    --categorical-fwer or --categorical-fwer-stepdown."""
    for text in _categorical_refusals(no_pairwise, collapse, False, names, labels):
        raise ValueError(text)
    for text in _cat_wy_refusals(fwer, True, permutations):
        raise ValueError(text)
    for text in _cat_sd_refusals(stepdown, True, permutations):
        raise ValueError(text)
    table = _as_table(genedic)
    eng = get_engine()
    N = len(table.strains)
    strata = np.asarray(strata)
    if len(labels) != len(names) or any(len(row) != N for row in labels):
        raise ValueError("categorical traits: labels must be [%d traits, %d isolates]" % (len(names), N))
    _side_stage_limits("categorical", eng, N, strata)
    classes, codes = _class_codes(labels, N)
    genes = table.on_device(eng)
    plan = eng.gcmh_plan(codes, strata)
    res = eng.gcmh(genes, plan)
    permutations = int(permutations)
    r = r_fwer = r_sd = None
    if stepdown:
        r, r_fwer, r_sd = (x.cpu().numpy() for x in eng.gcmh_stepdown(genes, plan, res, permutations, seed)[:3])
        r_fwer = r_fwer if fwer else None
    elif fwer:
        r, r_fwer = (x.cpu().numpy() for x in eng.gcmh_westfall_young(genes, plan, res, permutations, seed)[:2])
    elif permutations >= 10:
        r = eng.gcmh_permute(genes, plan, res, permutations, seed).cpu().numpy()
    a, e, m, q, df, p = (res[k].cpu().numpy() for k in ("a", "e", "m", "q", "df", "p"))
    out = {}
    for t, name in enumerate(names):
        K = len(classes[t])
        out[name] = dict(classes=classes[t], n=int(plan.n[t]), strata=int((plan.nsk_host[t].sum(axis=1) > 0).sum()),
                         a=a[t][:, :K], e=e[t][:, :K], m=m[t], q=q[t], df=df[t], p=p[t], testable=df[t] > 0)
        if r is not None:
            out[name]["r"] = r[t]
            out[name]["permutations"] = permutations
        if r_fwer is not None:
            out[name]["r_fwer"] = r_fwer[t]
        if r_sd is not None:
            out[name]["r_sd"] = r_sd[t]
        log.info("Generalized CMH test of %s: %d isolates with a label in %d classes and %d strata, %d genes tested"
                 % (name, out[name]["n"], K, out[name]["strata"], int(out[name]["testable"].sum())))
    return out


def most_enriched_expected(a, e):
    """The index of the class with the largest a_k / E_k over E_k > 0 (fp64 quotients); ties go to the first class."""
    best, top = None, -1.0
    for k, (ak, ek) in enumerate(zip(a, e)):
        if ek > 0.0 and float(ak) / float(ek) > top:
            best, top = k, float(ak) / float(ek)
    return best


def StoreGcmhResults(results, genedic, max_hits, outdir, time="", delimiter=",", stepdown=False):
    """Write ``<outdir><trait><time>.gcmh.results.csv`` for every trait of Gcmh_results, by StoreCategoricalResults'
    rules: the testable genes in ascending GCMH_p (ties in file order), Bonferroni and Benjamini-Hochberg over them,
    every cell double-quoted; ``stepdown`` as there.  Returns the file names."""
    def cells(res, g):
        a, e = res["a"][g], res["e"][g]
        return ["|".join("%s=%d" % (c, int(x)) for c, x in zip(res["classes"], a)),
                "|".join("%s=%s" % (c, _fmt(x)) for c, x in zip(res["classes"], e)),
                res["classes"][most_enriched_expected(a, e)], _fmt(res["q"][g]), _fmt(res["df"][g]), _fmt(res["p"][g])]
    return _store_side_results(results, genedic, max_hits, outdir, time, delimiter, GCMH_COLUMNS, cells,
                               ".gcmh.results.csv", "generalized CMH", stepdown=stepdown)


# ---------------------------------------------------------------------------
# --categorical-fwer: Westfall-Young single-step maxT over the chi-square and the generalized CMH statistic (spec
# S22): one more column, Westfall_Young_p, behind Empirical_p in the chi-square file and -- with --categorical-strata
# -- the generalized CMH file.  Nothing of the binary step's option tables (FLAG_RULES, OPTIONAL_COLUMNS) knows of it.
# ---------------------------------------------------------------------------
# a refusal, worded alike on the command line and in Categorical_results / Gcmh_results (fwer=True)
CAT_WY_TEXT = {
    "categorical": "Cannot use --categorical-fwer without --categorical. It is the family-wise p of the tests of the "
                   "categorical traits",
    "permute": "Cannot use --categorical-fwer without --permute X, X >= 10. The family-wise p is counted over the "
               "permutations of the labels",
}


def _cat_wy_refusals(fwer, categorical, permutations):
    """The messages of the --categorical-fwer rules that a run breaks, in the order they are reported."""
    if fwer and not categorical:
        yield CAT_WY_TEXT["categorical"]
    if fwer and int(permutations or 0) < 10:
        yield CAT_WY_TEXT["permute"]


# ---------------------------------------------------------------------------
# --categorical-fwer-stepdown: Westfall-Young step-down maxT over the chi-square and the generalized CMH statistic
# (spec S23): the column Westfall_Young_stepdown_p, the last of the chi-square file and -- with --categorical-strata
# -- the generalized CMH file, behind Westfall_Young_p where --categorical-fwer is given too.  Either flag works
# without the other.
# ---------------------------------------------------------------------------
CAT_SD_TEXT = {
    "categorical": "Cannot use --categorical-fwer-stepdown without --categorical. It is the step-down family-wise p "
                   "of the tests of the categorical traits",
    "permute": "Cannot use --categorical-fwer-stepdown without --permute X, X >= 10. The family-wise p is counted "
               "over the permutations of the labels",
}
# (rule, the run breaks it): in the order they are reported
CAT_SD_FLAG_RULES = (
    ("categorical", lambda categorical, permutations: not categorical),
    ("permute", lambda categorical, permutations: int(permutations or 0) < 10),
)


def _cat_sd_refusals(stepdown, categorical, permutations):
    """The messages of the --categorical-fwer-stepdown rules that a run breaks, in the order they are reported."""
    for key, broken in CAT_SD_FLAG_RULES:
        if stepdown and broken(categorical, permutations):
            yield CAT_SD_TEXT[key]


# ---------------------------------------------------------------------------
# --quantitative-strata FILE: the van Elteren test of the measured traits over strata (spec S16), next to the
# rank-sum stage: result files of its own, and nothing of the rank-sum files changes.
# ---------------------------------------------------------------------------
VANELTEREN_COLUMNS = ("Number_with_gene", "Number_without_gene", "Van_Elteren_AUC", "Van_Elteren_p", "Bonferroni_p",
                      "Benjamini_H_p")
VANELTEREN_TEXT = {
    "quantitative": "Cannot use --quantitative-strata without --quantitative. Its strata are those of the van Elteren "
                    "test of the measured traits",
    "file": "Could not find the strata file of --quantitative-strata: %s",
    "strata": "The strata file %s names %d strata for the analysed isolates; --quantitative-strata takes at most %d",
}


def VanElteren_results(genedic, names, values, strata, permutations=0, seed=DEFAULT_SEED, no_pairwise=True,
                       collapse=False, fwer=False, stepdown=False):
    """The van Elteren stage (spec S16) of the traits ``names`` with the values float64 [T, N] (nan = missing) and
    the stratum index of every isolate ``strata`` (N integers) over the isolates of ``genedic``: {name: dict(n,
    strata (those with a value), m, auc, p, var, testable [G]; r [G] with permutations >= 10; r_fwer [G] with
    ``fwer``, spec S17; r_sd [G] with ``stepdown``, spec S18)}, arrays in the gene table's order.  Raises ValueError
    where the command line refuses --quantitative, --quantitative-fwer or --quantitative-fwer-stepdown."""
    for text in _ranksum_refusals(no_pairwise, collapse, False):
        raise ValueError(text)
    for text in _rank_wy_refusals(fwer, True, permutations):
        raise ValueError(text)
    for text in _rank_sd_refusals(stepdown, True, permutations):
        raise ValueError(text)
    table = _as_table(genedic)
    eng = get_engine()
    values = np.asarray(values, dtype=np.float64)
    strata = np.asarray(strata)
    if values.ndim != 2 or values.shape != (len(names), len(table.strains)):
        raise ValueError("quantitative traits: values must be [%d traits, %d isolates]"
                         % (len(names), len(table.strains)))
    _side_stage_limits("quantitative", eng, len(table.strains), strata)
    genes = table.on_device(eng)
    plan = eng.vanelteren_plan(values, strata)
    res = eng.vanelteren(genes, plan)
    permutations = int(permutations)
    r = r_fwer = r_sd = None
    if stepdown:
        r, r_fwer, r_sd = (x.cpu().numpy() for x in eng.vanelteren_stepdown(genes, plan, res, permutations, seed)[:3])
        r_fwer = r_fwer if fwer else None
    elif fwer:
        r, r_fwer = (x.cpu().numpy() for x in eng.vanelteren_westfall_young(genes, plan, res, permutations, seed)[:2])
    elif permutations >= 10:
        r = eng.vanelteren_permute(genes, plan, res["d"], permutations, seed).cpu().numpy()
    m, auc, p, var = (res[k].cpu().numpy() for k in ("m", "auc", "p", "var"))
    out = {}
    for t, name in enumerate(names):
        out[name] = dict(n=int(plan.n[t].sum()), strata=int((plan.n[t] > 0).sum()), m=m[t], auc=auc[t], p=p[t],
                         var=var[t], testable=var[t] > 0)
        if r is not None:
            out[name]["r"] = r[t]
            out[name]["permutations"] = permutations
        if r_fwer is not None:
            out[name]["r_fwer"] = r_fwer[t]
        if r_sd is not None:
            out[name]["r_sd"] = r_sd[t]
        log.info("Van Elteren test of %s: %d isolates with a value in %d strata, %d genes tested"
                 % (name, out[name]["n"], out[name]["strata"], int(out[name]["testable"].sum())))
    return out


def StoreVanElterenResults(results, genedic, max_hits, outdir, time="", delimiter=","):
    """Write ``<outdir><trait><time>.vanelteren.results.csv`` for every trait of VanElteren_results, by
    StoreRanksumResults' rules: the testable genes in ascending Van_Elteren_p (ties in file order), Bonferroni and
    Benjamini-Hochberg over them, every cell double-quoted.  Returns the file names."""
    return _store_side_results(results, genedic, max_hits, outdir, time, delimiter, VANELTEREN_COLUMNS, _rank_cells,
                               ".vanelteren.results.csv", "van Elteren", rank=True)


# ---------------------------------------------------------------------------
# --quantitative-fwer: Westfall-Young single-step maxT over the rank statistics (spec S17): one more column,
# Westfall_Young_p, behind Empirical_p in the rank-sum file and -- with --quantitative-strata -- the van Elteren
# file.  Nothing of the binary step's option tables (FLAG_RULES, OPTIONAL_COLUMNS) knows of it.
# ---------------------------------------------------------------------------
# a refusal, worded alike on the command line and in Ranksum_results / VanElteren_results (fwer=True)
RANK_WY_TEXT = {
    "quantitative": "Cannot use --quantitative-fwer without --quantitative. It is the family-wise p of the rank tests "
                    "of the measured traits",
    "permute": "Cannot use --quantitative-fwer without --permute X, X >= 10. The family-wise p is counted over the "
               "permutations of the values",
}


def _rank_wy_refusals(fwer, quantitative, permutations):
    """The messages of the --quantitative-fwer rules that a run breaks, in the order they are reported."""
    if fwer and not quantitative:
        yield RANK_WY_TEXT["quantitative"]
    if fwer and int(permutations or 0) < 10:
        yield RANK_WY_TEXT["permute"]


# ---------------------------------------------------------------------------
# --quantitative-fwer-stepdown: Westfall-Young step-down maxT over the rank statistics (spec S18): the column
# Westfall_Young_stepdown_p, the last of the rank-sum file and -- with --quantitative-strata -- the van Elteren file,
# behind Westfall_Young_p where --quantitative-fwer is given too.  Either flag works without the other.
# ---------------------------------------------------------------------------
RANK_SD_TEXT = {
    "quantitative": "Cannot use --quantitative-fwer-stepdown without --quantitative. It is the step-down family-wise "
                    "p of the rank tests of the measured traits",
    "permute": "Cannot use --quantitative-fwer-stepdown without --permute X, X >= 10. The family-wise p is counted "
               "over the permutations of the values",
}
# (rule, the run breaks it): in the order they are reported
RANK_SD_FLAG_RULES = (
    ("quantitative", lambda quantitative, permutations: not quantitative),
    ("permute", lambda quantitative, permutations: int(permutations or 0) < 10),
)


def _rank_sd_refusals(stepdown, quantitative, permutations):
    """The messages of the --quantitative-fwer-stepdown rules that a run breaks, in the order they are reported."""
    for key, broken in RANK_SD_FLAG_RULES:
        if stepdown and broken(quantitative, permutations):
            yield RANK_SD_TEXT[key]


# ---------------------------------------------------------------------------
# --quantitative-shift: the Hodges-Lehmann shift of the rank-sum test and its confidence limits (spec S19): three
# columns of the rank-sum file, behind Benjamini_H_p and in front of Empirical_p, so that the Westfall-Young columns
# stay last.  No permutations; nothing of the van Elteren file changes.
# ---------------------------------------------------------------------------
RANK_SHIFT_LEVEL = 0.95
# (column, key of Ranksum_results' dict), in file order
RANK_SHIFT_COLUMNS = (("Rank_sum_shift", "shift"), ("Rank_sum_shift_lower", "shift_lower"),
                      ("Rank_sum_shift_upper", "shift_upper"))
RANK_SHIFT_TEXT = {
    "quantitative": "Cannot use --quantitative-shift without --quantitative. It is the shift of the measured traits "
                    "with a gene, next to the rank-sum test",
    "level_flag": "Cannot use --quantitative-shift-level without --quantitative-shift. It is the confidence level of "
                  "the limits of the Hodges-Lehmann shift",
    "level": "The confidence level of --quantitative-shift-level must be between 0.0 and 1.0 (both excluded)",
    "magnitude": "Cannot use --quantitative-shift with a value above 1e150 in magnitude: the difference of two such "
                 "values could overflow",
}
# (rule, the run breaks it): in the order they are reported.  ``level`` is None where none was given.
RANK_SHIFT_FLAG_RULES = (
    ("quantitative", lambda shift, quantitative, level, values: shift and not quantitative),
    ("level_flag", lambda shift, quantitative, level, values: level is not None and not shift),
    ("level", lambda shift, quantitative, level, values: level is not None and not 0.0 < float(level) < 1.0),
    ("magnitude", lambda shift, quantitative, level, values: shift and values is not None and _beyond_shift(values)),
)


def _beyond_shift(values):
    from .engine import SHIFT_MAX_ABS
    values = np.asarray(values, dtype=np.float64)
    return bool(np.any(np.abs(values[~np.isnan(values)]) > SHIFT_MAX_ABS))


def _rank_shift_refusals(shift, quantitative, level, values=None):
    """The messages of the --quantitative-shift rules that a run breaks, in the order they are reported, worded alike
    on the command line and in Ranksum_results (shift=True).  ``values``: the measured values, once they are read."""
    for key, broken in RANK_SHIFT_FLAG_RULES:
        if broken(shift, quantitative, level, values):
            yield RANK_SHIFT_TEXT[key]


def _shift_level(args):
    level = getattr(args, "quantitative_shift_level", None)
    return RANK_SHIFT_LEVEL if level is None else level


# ---------------------------------------------------------------------------
# --covariates FILE: covariate-adjusted score tests (spec S24).  The logistic score test of every binary trait of
# the traits file and, with --quantitative, the linear score test of every measured trait, each next to the file's
# up to eight numeric columns.  Stages and result files of their own, no permutation columns: labels are not
# exchangeable given continuous covariates.
# ---------------------------------------------------------------------------
LOGISTIC_COLUMNS = ("Number_with_gene", "Number_without_gene", "Beta", "Std_err", "Odds_ratio", "Score_chi2",
                    "Score_p", "Bonferroni_p", "Benjamini_H_p")
LINEAR_COLUMNS = ("Number_with_gene", "Number_without_gene", "Beta", "Std_err", "T_stat", "Linear_p", "Bonferroni_p",
                  "Benjamini_H_p")
# a refusal as the command line reports it / as Score_results raises it
SCORE_TEXT = {
    "no_pairwise": ("Cannot use --covariates without --no_pairwise. The score test is a test of every gene; the "
                    "covariates are its answer to population structure",
                    "covariates need no_pairwise: the score test is a test of every gene"),
    "collapse": ("Cannot use --covariates together with --collapse. The score test is a test of every gene of the "
                 "table", "covariates exclude collapse"),
    "ranks": ("Cannot use --covariates under more than one rank: the test runs over all genes in a single process",
              "covariates need a single process"),
    "columns": ("Cannot use --covariates with the %d columns of %s: the score test adjusts for at most %d. Keep the "
                "leading axes of the structure and the confounders that matter",
                "%d covariates (%s), at most %d are taken"),
    "isolates": ("The covariates file %s names none of the analysed isolates",
                 "the covariates (%s) are missing for every isolate"),
}
# --covariates-spa [--covariates-spa-cutoff X]: the saddlepoint-corrected p (spec S25), four last columns of the
# logistic files.  Its refusals, as SCORE_TEXT has them: the command line's exit message / Score_results' ValueError.
SCORE_SPA_COLUMNS = ("SPA_p", "SPA_Bonferroni_p", "SPA_Benjamini_H_p", "SPA_status")
SCORE_SPA_CUTOFF, SCORE_SPA_MIN_CUTOFF = 2.0, 0.1
SCORE_SPA_TEXT = {
    "covariates": ("Cannot use --covariates-spa without --covariates. The saddlepoint p corrects the logistic score "
                   "test of --covariates FILE", "the saddlepoint p needs the covariates' logistic score test"),
    "kind": ("Cannot use --covariates-spa for the linear score test", "the saddlepoint p belongs to the logistic score "
             "test: the linear one's t test is exact under its model"),
    "alone": ("Cannot use --covariates-spa-cutoff without --covariates-spa",
              "a saddlepoint cutoff without the saddlepoint p"),
    "cutoff": ("Cannot use --covariates-spa-cutoff %s: the cutoff is a finite number of at least %s standard "
               "deviations (default %s)", "the saddlepoint cutoff %s is not a finite number of at least %s (default %s)"),
}
# the one warning line of a trait whose null model S24 refuses (engine.SCORE_SKIPS says why)
SCORE_SKIPPED = "WARNING: Skipping the %s score test of %s: %s. No results file is written for it."


def _score_refusals(no_pairwise, collapse, names=None, covariates=None, source="", exits=False):
    """The messages of the --covariates rules that a run breaks, in the order they are reported (``exits``: as the
    command line's exit messages, else as Score_results' ValueErrors).  ``names`` and ``covariates`` ([c, N], nan =
    missing), where they are known: the rules on the file itself, ``source`` its path."""
    if not no_pairwise:
        yield SCORE_TEXT["no_pairwise"][not exits]
    if collapse:
        yield SCORE_TEXT["collapse"][not exits]
    from . import _abi, dist
    if dist.world_rank()[0] > 1:
        yield SCORE_TEXT["ranks"][not exits]
    if names is not None and len(names) > _abi.SCORE_MAX_COVARIATES:
        yield SCORE_TEXT["columns"][not exits] % ((len(names), source, _abi.SCORE_MAX_COVARIATES) if exits else
                                                  (len(names), ", ".join(names), _abi.SCORE_MAX_COVARIATES))
    if covariates is not None and len(covariates) and not (~np.isnan(np.asarray(covariates))).any():
        yield SCORE_TEXT["isolates"][not exits] % (source if exits else ", ".join(names or []))


def _score_spa_refusals(covariates, spa, cutoff, kind="logistic", exits=False):
    """The messages of the --covariates-spa rules that a run breaks, in the order they are reported (``exits`` as in
    _score_refusals): ``covariates`` = the score test runs, ``spa`` the flag, ``cutoff`` its cutoff or None."""
    if spa and not covariates:
        yield SCORE_SPA_TEXT["covariates"][not exits]
    if spa and kind != "logistic":
        yield SCORE_SPA_TEXT["kind"][not exits]
    if cutoff is not None and not spa:
        yield SCORE_SPA_TEXT["alone"][not exits]
    if cutoff is not None and not (np.isfinite(cutoff) and cutoff >= SCORE_SPA_MIN_CUTOFF):
        yield SCORE_SPA_TEXT["cutoff"][not exits] % (_fmt(float(cutoff)), SCORE_SPA_MIN_CUTOFF, SCORE_SPA_CUTOFF)


def read_covariates_file(path, delimiter, strains):
    """--covariates FILE: the layout of the --quantitative file, a header row (its first cell is ignored, the others
    name the covariates), then one row per isolate: its name and one cell per covariate, a finite number or one of
    MISSING_TRAIT.  Returns (names, float64 [c, N] over ``strains`` with nan = missing)."""
    def number(text, path, iso, column, line):
        try:
            x = float(text)
        except ValueError:
            x = np.nan
        if not np.isfinite(x):
            sys.exit("The covariates file %s has the cell %r for isolate %s, covariate %s (line %d): a cell is a "
                     "finite number or one of %s" % (path, text, iso, column, line,
                                                     ",".join(repr(m) for m in MISSING_TRAIT)))
        return x
    return _read_side_traits(path, delimiter, strains, "covariates", number,
                             lambda T, N: np.full((T, N), np.nan, dtype=np.float64))


def binary_trait_values(traitsdic, strains):
    """The traits of the traits file as the score test takes them: (names, float64 [T, N] over ``strains``: 1.0, 0.0
    or nan for an isolate without a value)."""
    names = list(traitsdic)
    values = np.full((len(names), len(strains)), np.nan, dtype=np.float64)
    for t, name in enumerate(names):
        for i, s in enumerate(strains):
            v = traitsdic[name].get(s)
            if v in ("0", "1"):
                values[t, i] = float(v)
    return names, values


def Score_results(genedic, names, values, covariate_names, covariates, kind="logistic", no_pairwise=True,
                  collapse=False, spa=False, spa_cutoff=None):
    """The score-test stage (spec S24) of the traits ``names`` with the values float64 [T, N] (nan = missing; 0 / 1
    for ``kind`` "logistic") next to the covariates float64 [c, N] over the isolates of ``genedic``: {name: dict(n,
    kind, m, beta, se, stat, p, testable [G])}, arrays in the gene table's order.  A trait whose null model S24
    refuses gets one warning line and no entry.  With ``spa`` (logistic kind only; spec S25) every entry also has
    spa_p float64 [G] and spa_status int32 [G], the saddlepoint-corrected p at the cutoff ``spa_cutoff`` (None: 2.0)
    and how it came about (0: below the cutoff, Score_p; 1: the saddlepoint p; 2: none could be formed, Score_p).
    Raises ValueError where the command line refuses --covariates or --covariates-spa."""
    for text in _score_refusals(no_pairwise, collapse, list(covariate_names), covariates):
        raise ValueError(text)
    for text in _score_spa_refusals(True, spa, spa_cutoff, kind):
        raise ValueError(text)
    table = _as_table(genedic)
    eng = get_engine()
    values = np.asarray(values, dtype=np.float64)
    covariates = np.asarray(covariates, dtype=np.float64).reshape(len(covariate_names), -1)
    if values.ndim != 2 or values.shape != (len(names), len(table.strains)) or \
            covariates.shape[1] != len(table.strains):
        raise ValueError("covariates: values must be [%d traits, %d isolates] and the covariates [%d, %d]"
                         % (len(names), len(table.strains), len(covariate_names), len(table.strains)))
    from .engine import SCORE_SKIPS
    genes = table.on_device(eng)
    plan = eng.score_plan(values, covariates, kind)
    on_device = eng.score(genes, plan)
    res = {k: v.cpu().numpy() for k, v in on_device.items()}
    stat = res["t" if kind == "linear" else "stat"]
    cutoff = SCORE_SPA_CUTOFF if spa_cutoff is None else float(spa_cutoff)
    saddle = {k: v.cpu().numpy() for k, v in eng.score_spa(genes, plan, on_device, cutoff).items()} if spa else None
    out = {}
    for t, name in enumerate(names):
        n = int(plan.n[t])
        if plan.skipped[t] is not None:
            why = SCORE_SKIPS[plan.skipped[t]]
            log.warning(SCORE_SKIPPED % (kind, name, why % {"few": (n, plan.q, plan.q + 1), "constant": (n,),
                                                             "one_class": (n,)}.get(plan.skipped[t], ())))
            continue
        testable = (res["m"][t] > 0) & (res["m"][t] < n) & (res["Vg"][t] > 2.0 ** -26 * res["b"][t, :, 0])
        if kind == "linear":
            testable &= n - plan.q - 1 >= 1
        out[name] = dict(n=n, kind=kind, m=res["m"][t], beta=res["beta"][t], se=res["se"][t], stat=stat[t],
                         p=res["p"][t], testable=testable)
        log.info("%s score test of %s next to %d covariates: %d isolates with a value and every covariate, %d genes "
                 "tested" % (kind.capitalize(), name, plan.q - 1, n, int(testable.sum())))
        if spa:
            out[name].update(spa_p=saddle["p"][t], spa_status=saddle["status"][t])
            status = saddle["status"][t][testable]
            log.info("Saddlepoint p of %s: %d of its %d tested genes are at or above the cutoff of %s standard "
                     "deviations, %d of them fell back to Score_p" % (name, int((status != 0).sum()), len(status),
                                                                      _fmt(cutoff), int((status == 2).sum())))
    return out


def _odds(beta):
    with np.errstate(over="ignore"):
        return float(np.exp(beta))


def _logistic_cells(res, g):
    beta = float(res["beta"][g])
    return [_fmt(beta), _fmt(res["se"][g]), _fmt(_odds(beta)), _fmt(res["stat"][g]), _fmt(res["p"][g])]


def _linear_cells(res, g):
    return [_fmt(res["beta"][g]), _fmt(res["se"][g]), _fmt(res["stat"][g]), _fmt(res["p"][g])]


def _spa_last(res, idx):
    """The four last columns of a logistic file whose result carries the saddlepoint p (SCORE_SPA_COLUMNS): SPA_p,
    its Bonferroni and Benjamini-Hochberg adjustments over the same testable genes ``idx``, and the status."""
    if "spa_p" not in res:
        return [], []
    if not len(idx):
        return list(SCORE_SPA_COLUMNS), []
    p = res["spa_p"][idx]
    bonf, bh = bonferroni_bh(p, len(idx))
    return list(SCORE_SPA_COLUMNS), [[_fmt(p[k]), _fmt(bonf[k]), _fmt(bh[k]), _fmt(int(res["spa_status"][g]))]
                                     for k, g in enumerate(idx)]


def StoreScoreResults(results, genedic, max_hits, outdir, time="", delimiter=","):
    """Write ``<outdir><trait><time>.logistic.results.csv`` (or ``.linear.results.csv``) for every trait of
    Score_results: the testable genes in ascending p (ties in file order), Bonferroni and Benjamini-Hochberg over
    them, every cell double-quoted; the carrier counts are over the trait's valid isolates.  A logistic result with
    the saddlepoint p (Score_results' ``spa``) gets SCORE_SPA_COLUMNS as its last columns; the rows, their order (by
    Score_p) and the cut by ``max_hits`` are the same with and without them.  Returns the file names."""
    files = []
    for kind, columns, cells in (("logistic", LOGISTIC_COLUMNS, _logistic_cells),
                                 ("linear", LINEAR_COLUMNS, _linear_cells)):
        of_kind = {name: res for name, res in results.items() if res["kind"] == kind}
        files += _store_side_results(of_kind, genedic, max_hits, outdir, time, delimiter, columns, cells,
                                     ".%s.results.csv" % kind, "%s score test" % kind, last=_spa_last)
    return files


class _LevelCounter(logging.Handler):
    def __init__(self):
        super().__init__(logging.WARNING)
        self.n = {}

    def emit(self, record):
        self.n[record.levelname] = self.n.get(record.levelname, 0) + 1


def read_strata_file(path, delimiter=","):
    """--permute-strata FILE: a CSV with a header row; column 1 = isolate name, column 2 = stratum label (any
    non-empty string), further columns ignored.  Returns {isolate: label} in file order."""
    out = {}
    with open(path, "r", newline=None) as f:
        rows = csv.reader(f, skipinitialspace=True, delimiter=delimiter)
        next(rows, None)                                   # the header row
        for line, row in enumerate(rows, start=2):
            if not row or all(c.strip() == "" for c in row):
                continue
            name = row[0].strip()
            label = row[1].strip() if len(row) > 1 else ""
            if label == "":
                sys.exit("The strata file %s has an empty stratum label for isolate %s (line %d)"
                         % (path, name, line))
            if name in out:
                sys.exit("The strata file %s names isolate %s more than once (line %d)" % (path, name, line))
            out[name] = label
    return out


def strata_indices(strata_map, strains):
    """(int64 array: the stratum index of every isolate of ``strains``, the list of stratum labels): labels are
    numbered 0 ... S-1 in order of first appearance along ``strains``; isolates of the file that are not analysed
    are ignored."""
    missing = [s for s in strains if s not in strata_map]
    if missing:
        sys.exit("The strata file does not name a stratum for %d of the analysed isolates, e.g. %s"
                 % (len(missing), ", ".join(missing[:5])))
    index, out = {}, np.zeros(len(strains), dtype=np.int64)
    for i, s in enumerate(strains):
        out[i] = index.setdefault(strata_map[s], len(index))
    return out, list(index)


def _analysed_isolates(args):
    """The isolate columns of the gene table that the run analyses: its header from column -s on, restricted to
    the isolates of -r -- what Csv_to_dic_Roary keeps, read from the first line alone."""
    with open(args.genes, "r", newline=None) as f:
        header = next(csv.reader(f, skipinitialspace=True, delimiter=args.delimiter), [])
    strains = header[int(args.start_col) - 1:]
    if args.restrict_to is not None and os.path.isfile(args.restrict_to):
        with open(args.restrict_to, "r") as f:
            allowed = {iso for line in f for iso in line.rstrip().split(",")}
        strains = [s for s in strains if s in allowed]
    return strains


def _strata_file_problems(args, flag, path):
    """What is wrong with the strata file ``path`` of ``flag`` (--cmh or --permute-strata), as exit messages."""
    if not os.path.isfile(path):
        yield "Could not find the strata file: %s" % path
    other = getattr(args, "permute_strata", None) if flag == "--cmh" else None
    if other and not (os.path.isfile(other) and os.path.samefile(other, path)):
        yield ("--cmh %s and --permute-strata %s name different strata files. With --cmh the permutations "
               "shuffle the labels within the strata of its file: give one file" % (path, other))


def _validate(args, cutoffs):
    """Argument checks of methods.py:126-181 (same conditions, same exits)."""
    if args.traits is None or args.genes is None:
        sys.exit("The following arguments are required: -t/--traits, -g/--genes")
    if args.threads <= 0:
        sys.exit("Number of threads must be positive")
    if not os.path.isfile(args.traits):
        sys.exit("Could not find the traits file: %s" % args.traits)
    if not os.path.isfile(args.genes):
        sys.exit("Could not find the gene presence absence file: %s" % args.genes)
    if args.newicktree is not None and not os.path.isfile(args.newicktree):
        sys.exit("Could not find the custom tree file: %s" % args.newicktree)
    if not all(0.0 < p <= 1.0 for p in args.p_value_cutoff):
        sys.exit("P must be between 0.0 and 1.0 or exactly 1.0")
    if len(args.delimiter) > 1:
        sys.exit("Delimiter must be a single character string. There is no support for tab.")
    if len(args.p_value_cutoff) != len(args.correction) and len(args.p_value_cutoff) != 1:
        sys.exit("You can not use more p-value cutoffs than correction methods. Either provide "
                 "a single p-value that will be applied to all correction methods, or provide "
                 "exactly as many as the number of correction methods and in corresponding "
                 "sequence. e.g. -c I EPW -p 0.1 0.05 will apply an individual p-value cutoff "
                 "of 0.1 AND a pairwise comparisons p-value cutoff of 0.05.")
    for rule in ALL_RULES:
        value = getattr(args, rule.flag[2:].replace("-", "_"), None)
        if value:
            files = _strata_file_problems(args, rule.flag, value) if isinstance(value, str) else ()
            for text in _broken_rules(rule, args.no_pairwise, args.permute,
                                      getattr(args, "permute_early_abort", False), files,
                                      cmh=bool(getattr(args, "cmh", None))):
                sys.exit(text)
    if getattr(args, "quantitative", None):
        for text in _ranksum_refusals(args.no_pairwise, args.collapse, bool(getattr(args, "permute_strata", None)),
                                      exits=True):
            sys.exit(text)
        if not os.path.isfile(args.quantitative):
            sys.exit("Could not find the quantitative traits file: %s" % args.quantitative)
    if getattr(args, "categorical", None):
        for text in _categorical_refusals(args.no_pairwise, args.collapse,
                                          bool(getattr(args, "permute_strata", None)), exits=True):
            sys.exit(text)
        if not os.path.isfile(args.categorical):
            sys.exit("Could not find the categorical traits file: %s" % args.categorical)
        # the classes are those of the analysed isolates (the header of the gene table after -s and -r): counted
        # here, before the engine starts and the table is read
        names, labels = read_categorical_file(args.categorical, args.delimiter, _analysed_isolates(args))
        for text in _categorical_refusals(True, False, False, names, labels, exits=True):
            sys.exit(text)
    for text in _score_spa_refusals(bool(getattr(args, "covariates", None)), getattr(args, "covariates_spa", False),
                                    getattr(args, "covariates_spa_cutoff", None), exits=True):
        sys.exit(text)
    if getattr(args, "covariates", None):
        for text in _score_refusals(args.no_pairwise, args.collapse, exits=True):
            sys.exit(text)
        if not os.path.isfile(args.covariates):
            sys.exit("Could not find the covariates file: %s" % args.covariates)
        # the file's own rules, on the analysed isolates (the header of the gene table after -s and -r): checked
        # here, before the engine starts and the table is read
        names, covariates = read_covariates_file(args.covariates, args.delimiter, _analysed_isolates(args))
        for text in _score_refusals(True, False, names, covariates, source=args.covariates, exits=True):
            sys.exit(text)
    cstrata = getattr(args, "categorical_strata", None)
    if cstrata:
        if not getattr(args, "categorical", None):
            sys.exit(GCMH_TEXT["categorical"])
        if not os.path.isfile(cstrata):
            sys.exit(GCMH_TEXT["file"] % cstrata)
        args.categorical_strata_map = read_strata_file(cstrata, args.delimiter)
        from . import _abi
        labels = strata_indices(args.categorical_strata_map, _analysed_isolates(args))[1]
        if len(labels) > _abi.PERM_MAX_STRATA:
            sys.exit(GCMH_TEXT["strata"] % (cstrata, len(labels), _abi.PERM_MAX_STRATA))
    for text in _cat_wy_refusals(getattr(args, "categorical_fwer", False), bool(getattr(args, "categorical", None)),
                                 args.permute):
        sys.exit(text)
    for text in _cat_sd_refusals(getattr(args, "categorical_fwer_stepdown", False),
                                 bool(getattr(args, "categorical", None)), args.permute):
        sys.exit(text)
    qstrata = getattr(args, "quantitative_strata", None)
    if qstrata:
        if not getattr(args, "quantitative", None):
            sys.exit(VANELTEREN_TEXT["quantitative"])
        if not os.path.isfile(qstrata):
            sys.exit(VANELTEREN_TEXT["file"] % qstrata)
        args.quantitative_strata_map = read_strata_file(qstrata, args.delimiter)
        from . import _abi
        labels = strata_indices(args.quantitative_strata_map, _analysed_isolates(args))[1]
        if len(labels) > _abi.PERM_MAX_STRATA:
            sys.exit(VANELTEREN_TEXT["strata"] % (qstrata, len(labels), _abi.PERM_MAX_STRATA))
    for text in _rank_wy_refusals(getattr(args, "quantitative_fwer", False),
                                  bool(getattr(args, "quantitative", None)), args.permute):
        sys.exit(text)
    for text in _rank_sd_refusals(getattr(args, "quantitative_fwer_stepdown", False),
                                  bool(getattr(args, "quantitative", None)), args.permute):
        sys.exit(text)
    for text in _rank_shift_refusals(getattr(args, "quantitative_shift", False),
                                     bool(getattr(args, "quantitative", None)),
                                     getattr(args, "quantitative_shift_level", None)):
        sys.exit(text)
    level = getattr(args, "cmh_exact_level", None)
    if level is not None and not getattr(args, "cmh_exact_odds", False):
        sys.exit("Cannot use --cmh-exact-level without --cmh-exact-odds. It is the confidence level of the limits "
                 "of the exact conditional odds ratio")
    if level is not None and not 0.0 < level < 1.0:
        sys.exit("The confidence level of --cmh-exact-level must be between 0.0 and 1.0 (both excluded)")
    strata_flag = "--permute-strata" if getattr(args, "permute_strata", None) else "--cmh"
    strata_path = getattr(args, "permute_strata", None) or getattr(args, "cmh", None)
    if strata_path:
        args.strata_map = read_strata_file(strata_path, args.delimiter)
        # the isolates of the analysis are the header of the gene table (after -s and -r): checked here, before the
        # engine starts and the table is read
        strata, labels = strata_indices(args.strata_map, _analysed_isolates(args))
        from . import _abi
        if len(labels) > _abi.PERM_MAX_STRATA:
            sys.exit("The strata file %s names %d strata for the analysed isolates; %s takes at "
                     "most %d" % (strata_path, len(labels), strata_flag, _abi.PERM_MAX_STRATA))
        if len(strata) > _abi.PERM_STRATA_MAX_ISOLATES:
            sys.exit("%s takes at most %d isolates; this analysis has %d"
                     % (strata_flag, _abi.PERM_STRATA_MAX_ISOLATES, len(strata)))
    if "P" in cutoffs and args.permute == 0:
        sys.exit("Cannot use empirical p-values in filtration without performing "
                 "permutations. Use '--permute X' where X is a number equal to or larger than 10")
    if args.permute < 10 and args.permute != 0:
        sys.exit("The absolute minimum number of permutations is 10 (or 0 to deactivate)")
    if "P" in cutoffs and cutoffs["P"] < (1.0 / args.permute):
        sys.exit("Permutation cutoff too low for this number of permutations")
    if args.permute > 10000:
        log.info("Note: You have set Scoary to do a high number of permutations. "
                 "This may take a while.")
    if args.no_pairwise:
        # The reference also zeroes --permute here (methods.py:174-181) because
        # its permutations need the tree.  The Fisher-statistic permutations of
        # this build do not, so --permute stays active (documented extension).
        log.info("Performing no pairwise comparisons. Ignoring all tree related options "
                 "(user tree, population aware-correction).")
        args.newicktree = None
        for m in ("PW", "EPW"):
            cutoffs.pop(m, None)


if __name__ == "__main__":
    main()
