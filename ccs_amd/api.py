"""ctypes mirror of include/ccsx.h — the host side used by tests, bench.py and the smoke test.

The product is libccsx.so (hand-written HIP kernels for gfx950 + a C++ host behind a C ABI).  This
module only marshals numpy arrays into the C structs; it contains no algorithmic code and there is
NO CPU fallback: if the library is missing, loading raises, and if no GPU is usable, `Handle()` raises.

Reference interface this mirrors: the "Draft Stage"/"Polish Stage" GPU consumers of
docs/img/ccs-impl.png and the per-ZMW outputs of docs/faq/bam-output.md:9-30 (rq, np, ec, sn, zm).
"""
from __future__ import annotations

import ctypes as C
import weakref
import os
from dataclasses import dataclass, replace

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CCSX_LIB", os.path.join(_HERE, "libccsx.so"))

BAND, MAXPRED, WIN_CORE, WIN_OVERHANG, JMAX, IMAX, MAX_ITER, NCTX, NOBS = 64, 7, 22, 2, 31, 63, 8, 16, 12   # include/ccsx.h (tests/test_abi.py compares)

STATUS_NAMES = {
    0: "SUCCESS", 1: "TOO_FEW_PASSES", 2: "DRAFT_FAILURE", 3: "TOO_MANY_UNUSABLE", 4: "NON_CONVERGENT",
    5: "TOO_SHORT", 6: "TOO_LONG", 7: "LOW_RQ", 8: "EMPTY_WINDOW", 9: "CAPACITY", 10: "HETERODUPLEX",
    11: "DRAFT_TOO_DIFFERENT", 12: "INSUFFICIENT_SPANS", 13: "COVERAGE_DROPS", 14: "READS_FAILED_POLISHING",
}
HETERODUPLEX = 10   # CCSX_HETERODUPLEX: a ZMW the heteroduplex split kept out of the polish stage (ccsx_hd_request.split)


class Model(C.Structure):
    _fields_ = [
        ("name", C.c_char * 32),
        ("snr_lo", C.c_float), ("snr_hi", C.c_float),
        ("trans_poly", C.c_float * 4 * 3 * NCTX),
        ("em_match", C.c_float * NOBS * NCTX),
        ("em_branch", C.c_float * 3 * NCTX),
        ("em_stick", C.c_float * 3 * NCTX),
    ]


class Opts(C.Structure):
    _fields_ = [
        ("max_poa_cov", C.c_int32), ("min_passes", C.c_int32), ("top_passes", C.c_int32),
        ("min_length", C.c_int32), ("max_length", C.c_int32), ("min_rq", C.c_float),
        ("poa_slots", C.c_int32), ("hifi_kinetics", C.c_int32), ("disable_heuristics", C.c_int32), ("min_zscore", C.c_float), ("handles_per_device", C.c_int32), ("no_fallback_draft", C.c_int32), ("max_insertion_size", C.c_int32), ("serial_stages", C.c_int32), ("max_qv", C.c_int32),
    ]


class CBatch(C.Structure):
    _fields_ = [
        ("n_zmw", C.c_int32), ("n_reads", C.c_int32), ("n_bases", C.c_int64),
        ("zmw_id", C.POINTER(C.c_int32)), ("snr", C.POINTER(C.c_float)),
        ("read_off", C.POINTER(C.c_int32)), ("base_off", C.POINTER(C.c_int64)),
        ("bases", C.POINTER(C.c_uint8)), ("pw", C.POINTER(C.c_uint8)), ("ipd", C.POINTER(C.c_uint8)),
        ("flags", C.POINTER(C.c_uint8)),
    ]


class CResults(C.Structure):
    _fields_ = [
        ("n_zmw", C.c_int32), ("seq_capacity", C.c_int64),
        ("seq_off", C.POINTER(C.c_int64)), ("status", C.POINTER(C.c_int32)), ("seq_len", C.POINTER(C.c_int32)),
        ("seq", C.POINTER(C.c_uint8)), ("qual", C.POINTER(C.c_uint8)), ("raw_qv", C.POINTER(C.c_float)),
        ("rq", C.POINTER(C.c_float)), ("np", C.POINTER(C.c_int32)), ("ec", C.POINTER(C.c_float)),
        ("iters", C.POINTER(C.c_int32)), ("n_windows", C.POINTER(C.c_int32)),
        ("fi", C.POINTER(C.c_uint8)), ("fp", C.POINTER(C.c_uint8)), ("ri", C.POINTER(C.c_uint8)), ("rp", C.POINTER(C.c_uint8)),
        ("fn", C.POINTER(C.c_int32)), ("rn", C.POINTER(C.c_int32)),
    ]


class CDrafts(C.Structure):
    _fields_ = [
        ("n_zmw", C.c_int32), ("seq_capacity", C.c_int64), ("win_capacity", C.c_int64),
        ("seq_off", C.POINTER(C.c_int64)), ("win_off", C.POINTER(C.c_int64)), ("status", C.POINTER(C.c_int32)), ("len", C.POINTER(C.c_int32)),
        ("seq", C.POINTER(C.c_uint8)), ("backbone", C.POINTER(C.c_int32)), ("n_windows", C.POINTER(C.c_int32)), ("win_bounds", C.POINTER(C.c_int32)),
    ]


QV_ONLY = 1     # ccsx_polish_batch flag (CCSX_QV_ONLY)
POA_LOG_WORDS = 5   # CCSX_POA_LOG_WORDS: I, end score, end position, threaded, vertices after the pass


# ---- the heteroduplex finder (include/ccsx.h ccsx_hd_*; DESIGN.md §2 "Heteroduplex rule")
HD_MAX_SITES, HD_WIN_SITES = 16, 8
HD_UNTESTED, HD_DOUBLE_STRAND, HD_HETERODUPLEX = 0, 1, 2
HD_VERDICT_NAMES = {0: "UNTESTED", 1: "DOUBLE_STRAND", 2: "HETERODUPLEX"}


class HdOpts(C.Structure):
    _fields_ = [("min_strand_passes", C.c_int32), ("min_sites", C.c_int32), ("min_indel", C.c_int32), ("min_alt_frac", C.c_float),
                ("max_pvalue", C.c_double)]


class HdSite(C.Structure):
    _fields_ = [("column", C.c_int32), ("kind", C.c_int8), ("alt", C.c_int8), ("fwd_alt", C.c_uint8), ("fwd_n", C.c_uint8),
                ("rev_alt", C.c_uint8), ("rev_n", C.c_uint8), ("pad_", C.c_uint8 * 2), ("p", C.c_double)]


HD_SITE_DTYPE = np.dtype({"names": ["column", "kind", "alt", "fwd_alt", "fwd_n", "rev_alt", "rev_n", "p"],
                          "formats": [np.int32, np.int8, np.int8, np.uint8, np.uint8, np.uint8, np.uint8, np.float64],
                          "offsets": [0, 4, 5, 6, 7, 8, 9, 16], "itemsize": 24})


class CHdReport(C.Structure):
    _fields_ = [("n_zmw", C.c_int32), ("verdict", C.POINTER(C.c_int32)), ("n_sub_sites", C.POINTER(C.c_int32)),
                ("n_indel_sites", C.POINTER(C.c_int32)), ("n_listed", C.POINTER(C.c_int32)), ("min_p", C.POINTER(C.c_double)),
                ("sites", C.POINTER(HdSite)), ("status", C.POINTER(C.c_int32))]


class CHdRequest(C.Structure):
    """ccsx_hd_request: the heteroduplex finder in the fused path (ccsx_consensus_hd / ccsx_submit_hd)"""
    _fields_ = [("opts", C.POINTER(HdOpts)), ("report", C.POINTER(CHdReport)), ("split", C.c_int32), ("reserved", C.c_int32)]


def hd_opts_default() -> HdOpts:
    o = HdOpts()
    lib().ccsx_hd_opts_default(C.byref(o))
    return o


class _PlaneReport:
    """What the reports of the optional analyses share.  PLANES lists the arrays as (name, dtype, per-ZMW shape); each is an attribute of that name, [n_zmw, *shape],
    and the pointer of that name in CSTRUCT, the report's ctypes struct.  Plain classes, not dataclasses: built by allocate() or from the arrays in PLANES
    order, without keyword construction, __repr__ or field-wise __eq__ (compare the arrays); _pinned holds the page-locked blocks, empty when not pinned."""
    PLANES: tuple = ()
    CSTRUCT = None

    def __init__(self, *arrays):
        for (k, _, _), a in zip(self.PLANES, arrays, strict=True):
            setattr(self, k, a)

    @classmethod
    def allocate(cls, n: int, pinned: bool = False):
        """every array zeroed.  pinned=True: page-locked arrays (the ticketed form, Handle.submit, downloads into them asynchronously)"""
        keep = []

        def z(dt, shape):
            count = n * int(np.prod(shape, dtype=np.int64))
            a = _pinned_array(count, dt, keep) if pinned else np.empty(count, dt)
            a.view(np.uint8)[...] = 0
            return a.reshape((n,) + shape)
        rep = cls(*(z(dt, shape) for _, dt, shape in cls.PLANES))
        rep._pinned = keep
        return rep

    def c_struct(self):
        r = self.CSTRUCT()
        r.n_zmw = len(self.verdict)
        types = dict(self.CSTRUCT._fields_)
        for k, _, _ in self.PLANES:
            setattr(r, k, getattr(self, k).ctypes.data_as(types[k]))
        return r


def _int_planes(*names) -> tuple:
    return tuple((k, np.int32, ()) for k in names)


class HdReport(_PlaneReport):
    """ccsx_hd_report: one verdict per ZMW, the site counts and the listed sites (structured array [n_zmw, HD_MAX_SITES] of HD_SITE_DTYPE)."""
    PLANES = _int_planes("verdict", "n_sub_sites", "n_indel_sites", "n_listed") + (("min_p", np.float64, ()), ("sites", HD_SITE_DTYPE, (HD_MAX_SITES,))) \
        + _int_planes("status")
    CSTRUCT = CHdReport

    @classmethod
    def allocate(cls, n: int, pinned: bool = False) -> "HdReport":
        rep = super().allocate(n, pinned)
        rep.min_p[...] = 1.0
        return rep

    def site_list(self, z: int) -> np.ndarray:
        return self.sites[z, : int(self.n_listed[z])]


# ---- adapter palindromes (include/ccsx.h ccsx_fold_*; DESIGN.md §2 "Adapter palindromes")
FOLD_UNTESTED, FOLD_NONE, FOLD_PALINDROME = 0, 1, 2


class FoldOpts(C.Structure):
    _fields_ = [("max_occ", C.c_int32), ("min_hits", C.c_int32), ("min_arm", C.c_int32), ("min_span_tenths", C.c_int32), ("end_slack", C.c_int32)]


class CFoldReport(C.Structure):
    _fields_ = [("n_zmw", C.c_int32), ("verdict", C.POINTER(C.c_int32)), ("fold", C.POINTER(C.c_int32)), ("hits", C.POINTER(C.c_int32)),
                ("span", C.POINTER(C.c_int32))]


class CFoldRequest(C.Structure):
    """ccsx_fold_request: adapter-palindrome detection in the fused path (ccsx_consensus_fold / ccsx_submit_fold)"""
    _fields_ = [("opts", C.POINTER(FoldOpts)), ("report", C.POINTER(CFoldReport)), ("reserved", C.c_int32 * 2)]


def fold_opts_default() -> FoldOpts:
    o = FoldOpts()
    lib().ccsx_fold_opts_default(C.byref(o))
    return o


class FoldReport(_PlaneReport):
    """ccsx_fold_report: per ZMW the verdict (FOLD_*), the fold centre in draft coordinates (-1: no hit), the hits and the span of the winning bins."""
    PLANES = _int_planes("verdict", "fold", "hits", "span")
    CSTRUCT = CFoldReport


def _fold_request(opts: "FoldOpts | None", crep: CFoldReport) -> tuple[CFoldRequest, FoldOpts]:
    o = opts if opts is not None else fold_opts_default()
    return CFoldRequest(C.pointer(o), C.pointer(crep), (C.c_int32 * 2)(0, 0)), o


# ---- adapter screen (include/ccsx.h ccsx_adapter_*; DESIGN.md §2 "Adapter screen")
ADAPTER_CONCAT, ADAPTER_NEAR_END = 1, 2
ADAPTER_MAX_PATTERNS, ADAPTER_MIN_LEN, ADAPTER_MAX_LEN, ADAPTER_MAX_HITS = 8, 16, 64, 16
ADAPTER_HIT = np.dtype([("start", np.int32), ("end", np.int32), ("search", np.uint8), ("dist", np.uint8), ("pad_", np.uint8, 2)])


class AdapterOpts(C.Structure):
    _fields_ = [("max_dist_pct", C.c_int32), ("min_copies", C.c_int32), ("max_insert", C.c_int32), ("end_slack", C.c_int32)]


class AdapterSet(C.Structure):
    """ccsx_adapter_set: up to 8 adapters of 16 .. 64 codes 0 .. 3; each is searched as given and as its reverse complement"""
    _fields_ = [("n_adapters", C.c_int32), ("len", C.c_int32 * ADAPTER_MAX_PATTERNS), ("seq", (C.c_uint8 * ADAPTER_MAX_LEN) * ADAPTER_MAX_PATTERNS)]

    @staticmethod
    def from_strings(seqs) -> "AdapterSet":
        """from ACGT strings (either case) or arrays of codes; lengths and the count are checked by the call that takes the set"""
        seqs = list(seqs)
        if len(seqs) > ADAPTER_MAX_PATTERNS:
            raise ValueError(f"at most {ADAPTER_MAX_PATTERNS} adapters")
        s = AdapterSet()
        s.n_adapters = len(seqs)
        for a, q in enumerate(seqs):
            codes = ["ACGT".index(c) for c in q.upper()] if isinstance(q, str) else [int(c) for c in q]
            if len(codes) > ADAPTER_MAX_LEN:
                raise ValueError(f"adapter {a}: more than {ADAPTER_MAX_LEN} bases")
            s.len[a] = len(codes)
            for i, c in enumerate(codes):
                s.seq[a][i] = c
        return s

    @staticmethod
    def default() -> "AdapterSet":
        s = AdapterSet()
        if lib().ccsx_adapter_set_default(C.byref(s)) != 0:
            raise RuntimeError("ccsx_adapter_set_default failed")
        return s

    def strings(self) -> list:
        return ["".join("ACGT"[self.seq[a][i]] for i in range(self.len[a])) for a in range(self.n_adapters)]


class CAdapterReport(C.Structure):
    _fields_ = [("n_zmw", C.c_int32)] + [(k, C.POINTER(C.c_int32)) for k in ("tested", "verdict", "n_hits", "n_listed", "covered", "max_gap", "first_start",
                                                                              "last_end", "min_dist")] + [("hits", C.c_void_p)]


class CAdapterRequest(C.Structure):
    """ccsx_adapter_request: the adapter screen in the fused path (ccsx_consensus_screen / ccsx_submit_screen)"""
    _fields_ = [("adapters", C.POINTER(AdapterSet)), ("opts", C.POINTER(AdapterOpts)), ("report", C.POINTER(CAdapterReport)), ("reserved", C.c_int32 * 2)]


def adapter_opts_default() -> AdapterOpts:
    o = AdapterOpts()
    lib().ccsx_adapter_opts_default(C.byref(o))
    return o


class AdapterReport(_PlaneReport):
    """ccsx_adapter_report: per ZMW tested (0 / 1), the verdict bits (ADAPTER_CONCAT | ADAPTER_NEAR_END), the aggregates over every hit, and the first 16 hits
    in increasing (end, search) as a structured array [n_zmw, 16] (ADAPTER_HIT)"""
    INT_FIELDS = ("tested", "verdict", "n_hits", "n_listed", "covered", "max_gap", "first_start", "last_end", "min_dist")
    PLANES = _int_planes(*INT_FIELDS) + (("hits", ADAPTER_HIT, (ADAPTER_MAX_HITS,)),)
    CSTRUCT = CAdapterReport

    def listed(self, z: int) -> list:
        """the listed hits of ZMW z as (start, end, search, dist)"""
        return [(int(h["start"]), int(h["end"]), int(h["search"]), int(h["dist"])) for h in self.hits[z, : int(self.n_listed[z])]]


def _adapter_request(aset: "AdapterSet | None", opts: "AdapterOpts | None", crep: CAdapterReport):
    a = aset if aset is not None else AdapterSet.default()
    o = opts if opts is not None else adapter_opts_default()
    return CAdapterRequest(C.pointer(a), C.pointer(o), C.pointer(crep), (C.c_int32 * 2)(0, 0)), (a, o)


# ---- control screen (include/ccsx.h ccsx_control_*; DESIGN.md §2 "Control screen")
CONTROL_UNTESTED, CONTROL_NONE, CONTROL_FOUND = 0, 1, 2
CONTROL_MIN_LEN, CONTROL_MAX_LEN = 64, 4096


class ControlOpts(C.Structure):
    _fields_ = [("max_occ", C.c_int32), ("min_matched", C.c_int32), ("min_ctl_tenths", C.c_int32), ("min_draft_tenths", C.c_int32)]


class ControlSeq(C.Structure):
    """ccsx_control_seq: the spike-in control, 64 .. 4096 codes 0 .. 3 (the length and the codes are checked by the call that takes it)"""
    _fields_ = [("len", C.c_int32), ("reserved", C.c_int32), ("seq", C.POINTER(C.c_uint8))]

    @staticmethod
    def from_codes(codes) -> "ControlSeq":
        a = np.ascontiguousarray(np.asarray(codes, np.uint8))
        s = ControlSeq(len(a), 0, _ptr(a, C.c_uint8))
        s._codes = a                                               # (the struct points into it)
        return s

    @staticmethod
    def from_string(seq: str) -> "ControlSeq":
        """from an ACGT string (either case)"""
        return ControlSeq.from_codes(["ACGT".index(c) for c in seq.upper()])

    def codes(self) -> np.ndarray:
        return np.ctypeslib.as_array(self.seq, (self.len,)).copy()


class CControlReport(C.Structure):
    _fields_ = [("n_zmw", C.c_int32)] + [(k, C.POINTER(C.c_int32)) for k in ("verdict", "strand", "hits", "matched", "ctl_start", "ctl_end", "draft_start",
                                                                              "draft_end")]


class CControlRequest(C.Structure):
    """ccsx_control_request: the control screen in the fused path (ccsx_consensus_control / ccsx_submit_control)"""
    _fields_ = [("control", C.POINTER(ControlSeq)), ("opts", C.POINTER(ControlOpts)), ("report", C.POINTER(CControlReport)), ("reserved", C.c_int32 * 2)]


def control_opts_default() -> ControlOpts:
    o = ControlOpts()
    lib().ccsx_control_opts_default(C.byref(o))
    return o


class ControlReport(_PlaneReport):
    """ccsx_control_report: per ZMW the verdict (CONTROL_*), the strand (-1: no hit), the hits of the winning pair of diagonal bins, the distinct control
    positions among them and the control and draft bases they span"""
    FIELDS = ("verdict", "strand", "hits", "matched", "ctl_start", "ctl_end", "draft_start", "draft_end")
    PLANES = _int_planes(*FIELDS)
    CSTRUCT = CControlReport


def _control_request(seq: ControlSeq, opts: "ControlOpts | None", crep: CControlReport):
    o = opts if opts is not None else control_opts_default()
    return CControlRequest(C.pointer(seq), C.pointer(o), C.pointer(crep), (C.c_int32 * 2)(0, 0)), (seq, o)


# ---- coverage screen (include/ccsx.h ccsx_coverage_*; DESIGN.md §2 "Coverage rule")
COVERAGE_UNTESTED, COVERAGE_NONE, COVERAGE_DRAFT_TOO_DIFFERENT, COVERAGE_INSUFFICIENT_SPANS, COVERAGE_COVERAGE_DROPS, COVERAGE_READS_FAILED_POLISHING = range(6)
COVERAGE_GATE_ALL = 0x3c                         # every gate bit: verdict v = 2 .. 5 -> status 9 + v
DRAFT_TOO_DIFFERENT, INSUFFICIENT_SPANS, COVERAGE_DROPS, READS_FAILED_POLISHING = 11, 12, 13, 14   # CCSX_* statuses of the gate


class CoverageOpts(C.Structure):
    _fields_ = [("drop_percent", C.c_int32), ("block", C.c_int32), ("min_spans", C.c_int32), ("max_lost_percent", C.c_int32)]


class CCoverageReport(C.Structure):
    _fields_ = [("n_zmw", C.c_int32)] + [(k, C.POINTER(C.c_int32)) for k in ("verdict", "np_aligned", "spans", "cov_max", "clean_min", "drop_window", "drop_windows",
                                                                              "reach_sum", "used_sum", "used_min")]


class CCoverageRequest(C.Structure):
    """ccsx_coverage_request: the coverage screen in the fused path (ccsx_consensus_requests / ccsx_submit_requests)"""
    _fields_ = [("opts", C.POINTER(CoverageOpts)), ("report", C.POINTER(CCoverageReport)), ("gate", C.c_uint32), ("reserved", C.c_int32 * 2)]


def coverage_opts_default() -> CoverageOpts:
    o = CoverageOpts()
    lib().ccsx_coverage_opts_default(C.byref(o))
    return o


class CoverageReport(_PlaneReport):
    """ccsx_coverage_report: per ZMW the verdict (COVERAGE_*) and the counts behind it.  PRE: the planes known before the polish, POST: those after it"""
    PRE = ("verdict", "np_aligned", "spans", "cov_max", "clean_min", "drop_window", "drop_windows")
    POST = ("reach_sum", "used_sum", "used_min")
    FIELDS = PRE + POST
    PLANES = _int_planes(*FIELDS)
    CSTRUCT = CCoverageReport


def _coverage_request(opts: "CoverageOpts | None", gate: int, crep: CCoverageReport):
    o = opts if opts is not None else coverage_opts_default()
    return CCoverageRequest(C.pointer(o), C.pointer(crep), int(gate), (C.c_int32 * 2)(0, 0)), o


# ---- polisher hand-off (include/ccsx.h ccsx_handoff_*; DESIGN.md §2 "Polisher hand-off")
HANDOFF_NO_BASE, HANDOFF_NO_SEGMENT = 4, 5       # cell base codes beside 0-3: no base of the pass on the column; no usable segment, row or column


class HandoffOpts(C.Structure):
    _fields_ = [("tile_len", C.c_int32), ("max_rows", C.c_int32), ("skip_above", C.c_int32), ("reserved", C.c_int32)]


class CHandoffOut(C.Structure):
    """ccsx_handoff_out: every array is host or device memory, so the mirror keeps plain addresses"""
    _fields_ = [("max_tiles", C.c_int64)] + [(k, C.c_void_p) for k in ("counts", "tile_zmw", "tile_start", "tile_len", "tile_qsum", "tile_rows", "row_pass",
                                                                     "row_strand", "cells")]


class CHandoffRequest(C.Structure):
    _fields_ = [("opts", C.POINTER(HandoffOpts)), ("out", C.POINTER(CHandoffOut)), ("reserved", C.c_int64 * 2)]


def handoff_opts_default() -> HandoffOpts:
    o = HandoffOpts()
    lib().ccsx_handoff_opts_default(C.byref(o))
    return o


def handoff_tile_bound(batch: "Batch", tile_len: int) -> int:
    """tiles a batch can have at most: every ZMW's consensus capacity (ccsx_result_layout) cut into tiles"""
    off = np.zeros(batch.n_zmw + 1, np.int64)
    cb = batch.c_struct()
    lib().ccsx_result_layout(C.byref(cb), _ptr(off, C.c_int64))
    return max(1, int(((np.diff(off) + tile_len - 1) // tile_len).sum()))


class Handoff:
    """ccsx_handoff_out with its options: the selected tiles of a batch as pass-by-column arrays.  counts [2] (tiles, selected tiles), tile_zmw / tile_start /
    tile_len / tile_qsum / tile_rows [max_tiles] int32, row_pass / row_strand [max_tiles, R] uint8, cells [max_tiles, R, T, 4] uint8 = (base, pw, ip, ins).
    The arrays are numpy (pageable or page-locked) or, with device=, torch tensors in the memory of that GPU: nothing of them crosses PCIe."""
    FIELDS = ("counts", "tile_zmw", "tile_start", "tile_len", "tile_qsum", "tile_rows", "row_pass", "row_strand", "cells")

    def __init__(self, opts: HandoffOpts, max_tiles: int, arrays: dict, on_device: bool, keep=None):
        self.opts, self.max_tiles, self.on_device, self._keep = opts, int(max_tiles), on_device, keep
        for k in self.FIELDS:
            setattr(self, k, arrays[k])

    @staticmethod
    def shapes(max_tiles: int, opts: HandoffOpts) -> dict:
        m, r, t = int(max_tiles), int(opts.max_rows), int(opts.tile_len)
        d = {k: ((m,), np.int32) for k in Handoff.FIELDS[1:6]}
        d.update(counts=((2,), np.int32), row_pass=((m, r), np.uint8), row_strand=((m, r), np.uint8), cells=((m, r, t, 4), np.uint8))
        return d

    @classmethod
    def allocate(cls, batch: "Batch", max_tiles: "int | None" = None, opts: "HandoffOpts | None" = None, pinned: bool = False,
                 device: "bool | int" = False) -> "Handoff":
        """max_tiles None: room for every tile the batch can have.  pinned=True: page-locked arrays (Handle.submit).  device=True (GPU 0) or a device
        ordinal: torch tensors on that GPU — it must be the handle's"""
        o = opts if opts is not None else handoff_opts_default()
        m = handoff_tile_bound(batch, int(o.tile_len)) if max_tiles is None else int(max_tiles)
        shapes = cls.shapes(max(m, 0), o)
        keep = []
        if device is not False:
            import torch
            dev = torch.device("cuda", 0 if device is True else int(device))
            dts = {np.int32: torch.int32, np.uint8: torch.uint8}
            arrays = {k: torch.zeros(sh, dtype=dts[dt], device=dev) for k, (sh, dt) in shapes.items()}
            torch.cuda.synchronize(dev)                      # the fills are done before the engine's own streams write
        elif pinned:
            arrays = {k: _pinned_array(int(np.prod(sh)), dt, keep).reshape(sh) for k, (sh, dt) in shapes.items()}
            for a in arrays.values():
                a[...] = 0
        else:
            arrays = {k: np.zeros(sh, dt) for k, (sh, dt) in shapes.items()}
        return cls(o, m, arrays, device is not False, keep)

    def c_struct(self) -> CHandoffOut:
        c = CHandoffOut()
        c.max_tiles = self.max_tiles
        for k in self.FIELDS:
            a = getattr(self, k)
            setattr(c, k, a.data_ptr() if self.on_device else a.ctypes.data)
        return c

    def host(self) -> "Handoff":
        """the same hand-off with numpy arrays (a device one is copied to the host; call after the run has ended)"""
        if not self.on_device:
            return self
        return Handoff(self.opts, self.max_tiles, {k: getattr(self, k).cpu().numpy() for k in self.FIELDS}, False)

    @property
    def n_tiles(self) -> int:
        """slots that were written: min(selected tiles, max_tiles)"""
        return min(int(self.counts[1]), self.max_tiles)

    def backbones(self, n_zmw: int) -> np.ndarray:
        """per ZMW a pass that has the orientation of SEQ, for Handle.refine: the row_pass of the first row with row_strand 0 among the ZMW's slots; -1 where the
        ZMW has no slot or no such row"""
        ho = self.host()
        bb = np.full(int(n_zmw), -1, np.int32)
        for g in range(ho.n_tiles):
            z = int(ho.tile_zmw[g])
            if bb[z] >= 0:
                continue
            for k in range(int(ho.tile_rows[g])):
                if ho.row_pass[g, k] != 255 and ho.row_strand[g, k] == 0:
                    bb[z] = int(ho.row_pass[g, k])
                    break
        return bb

    def tile(self, g: int) -> dict:
        """slot g: zmw, start, len, qsum, rows, row_pass [R], row_strand [R], cells [R, len, 4]"""
        if not 0 <= g < self.n_tiles:
            raise IndexError(f"tile {g} of {self.n_tiles}")
        ln = int(self.tile_len[g])
        return dict(zmw=int(self.tile_zmw[g]), start=int(self.tile_start[g]), len=ln, qsum=int(self.tile_qsum[g]), rows=int(self.tile_rows[g]),
                    row_pass=self.row_pass[g], row_strand=self.row_strand[g], cells=self.cells[g][:, :ln])


def _handoff_request(ho: Handoff):
    co = ho.c_struct()
    return CHandoffRequest(C.pointer(ho.opts), C.pointer(co), (C.c_int64 * 2)(0, 0)), co


# ---- polisher hand-back (include/ccsx.h ccsx_refine_*; DESIGN.md §2 "Polisher hand-back")
REFINE_SKIPPED, REFINE_RESCORED, REFINE_REFINED = 0, 1, 2
REFINE_BAD_TILE, REFINE_BAD_ORDER, REFINE_BAD_SYMBOL, REFINE_TOO_LONG, REFINE_EMPTY, REFINE_BAD_BACKBONE, REFINE_BAD_LIST = -1, -2, -3, -4, -5, -6, -7
REFINE_CODE_NAMES = {0: "SKIPPED", 1: "RESCORED", 2: "REFINED", -1: "BAD_TILE", -2: "BAD_ORDER", -3: "BAD_SYMBOL", -4: "TOO_LONG", -5: "EMPTY", -6: "BAD_BACKBONE",
                     -7: "BAD_LIST"}


class CRefineTiles(C.Structure):
    """ccsx_refine_tiles: every array is host or device memory, so the mirror keeps plain addresses"""
    _fields_ = [("n_tiles", C.c_int64), ("stride", C.c_int32), ("reserved0", C.c_int32)] + \
               [(k, C.c_void_p) for k in ("tile_zmw", "tile_start", "tile_len", "new_len", "new_seq", "new_qual")] + [("reserved", C.c_int64 * 2)]


class CRefineReport(C.Structure):
    _fields_ = [("counts", C.POINTER(C.c_int32)), ("code", C.POINTER(C.c_int32)), ("n_applied", C.POINTER(C.c_int32)), ("new_len", C.POINTER(C.c_int32)),
                ("rq_merged", C.POINTER(C.c_float)), ("qual_merged", C.POINTER(C.c_uint8))]


def refine_perr_table() -> np.ndarray:
    """the engine's perr_fx[0 .. 93] (ccsx_refine_perr), uint64"""
    return np.array([lib().ccsx_refine_perr(q) for q in range(94)], np.uint64)


class RefineTiles:
    """ccsx_refine_tiles: the second polisher's answer as replace-intervals on the consensus.  tile_zmw / tile_start / tile_len / new_len [n_tiles] int32,
    new_seq / new_qual [n_tiles, stride] uint8.  The arrays are numpy (pageable or page-locked) or, with device=, torch tensors in the memory of that GPU."""
    FIELDS = ("tile_zmw", "tile_start", "tile_len", "new_len", "new_seq", "new_qual")

    def __init__(self, n_tiles: int, stride: int, arrays: dict, on_device: bool, keep=None):
        self.n_tiles, self.stride, self.on_device, self._keep = int(n_tiles), int(stride), on_device, keep
        for k in self.FIELDS:
            setattr(self, k, arrays[k])

    @staticmethod
    def shapes(n_tiles: int, stride: int) -> dict:
        m, u = int(n_tiles), int(stride)
        d = {k: ((m,), np.int32) for k in RefineTiles.FIELDS[:4]}
        d.update(new_seq=((m, u), np.uint8), new_qual=((m, u), np.uint8))
        return d

    @classmethod
    def allocate(cls, n_tiles: int, stride: int = 128, device: "bool | int" = False, pinned: bool = False) -> "RefineTiles":
        """zeroed arrays.  device=True (GPU 0) or a device ordinal: torch tensors on that GPU — it must be the handle's; pinned=True: page-locked arrays"""
        shapes = cls.shapes(max(int(n_tiles), 0), stride)
        keep = []
        if device is not False:
            import torch
            dev = torch.device("cuda", 0 if device is True else int(device))
            dts = {np.int32: torch.int32, np.uint8: torch.uint8}
            arrays = {k: torch.zeros(sh, dtype=dts[dt], device=dev) for k, (sh, dt) in shapes.items()}
            torch.cuda.synchronize(dev)
        elif pinned:
            arrays = {k: _pinned_array(int(np.prod(sh)), dt, keep).reshape(sh) for k, (sh, dt) in shapes.items()}
            for a in arrays.values():
                a[...] = 0
        else:
            arrays = {k: np.zeros(sh, dt) for k, (sh, dt) in shapes.items()}
        return cls(n_tiles, stride, arrays, device is not False, keep)

    @classmethod
    def from_arrays(cls, tile_zmw, tile_start, tile_len, new_len, new_seq, new_qual, stride: "int | None" = None, device: "bool | int" = False,
                    pinned: bool = False) -> "RefineTiles":
        """new_seq / new_qual: [n_tiles, stride] arrays, or a list of per-tile sequences (then new_len may be None: their lengths) padded to `stride` [128]"""
        m = len(tile_zmw)
        if not isinstance(new_seq, np.ndarray) or new_seq.ndim != 2:
            rows_s, rows_q = [np.asarray(r, np.uint8) for r in new_seq], [np.asarray(r, np.uint8) for r in new_qual]
            u = int(stride) if stride is not None else 128
            if new_len is None:
                new_len = [len(r) for r in rows_s]
            new_seq, new_qual = np.zeros((m, u), np.uint8), np.zeros((m, u), np.uint8)
            for g in range(m):
                k = min(len(rows_s[g]), u)
                new_seq[g, :k], new_qual[g, :k] = rows_s[g][:k], rows_q[g][:k]
        u = int(stride) if stride is not None else (int(new_seq.shape[1]) if m else 128)
        t = cls.allocate(m, u, device=device, pinned=pinned)
        src = dict(tile_zmw=tile_zmw, tile_start=tile_start, tile_len=tile_len, new_len=new_len, new_seq=new_seq, new_qual=new_qual)
        for k, (sh, dt) in cls.shapes(m, u).items():
            a = np.ascontiguousarray(np.asarray(src[k]).astype(dt, copy=False).reshape(sh))
            if t.on_device:
                import torch
                getattr(t, k).copy_(torch.from_numpy(a))
            else:
                getattr(t, k)[...] = a
        if t.on_device:
            import torch
            torch.cuda.synchronize(getattr(t, "tile_zmw").device)    # the copies are done before the engine's own streams read
        return t

    def c_struct(self) -> CRefineTiles:
        c = CRefineTiles()
        c.n_tiles, c.stride = self.n_tiles, self.stride
        for k in self.FIELDS:
            a = getattr(self, k)
            setattr(c, k, (a.data_ptr() if self.on_device else a.ctypes.data) if self.n_tiles > 0 else None)
        return c

    def host(self) -> "RefineTiles":
        if not self.on_device:
            return self
        return RefineTiles(self.n_tiles, self.stride, {k: getattr(self, k).cpu().numpy() for k in self.FIELDS}, False)


class RefineReport:
    """ccsx_refine_report: counts [3] (ZMWs refined, tiles applied, list-order violations), code / n_applied / new_len [n] int32, rq_merged [n] float32,
    qual_merged [capacity] uint8 or None"""
    FIELDS = ("counts", "code", "n_applied", "new_len", "rq_merged", "qual_merged")

    def __init__(self, seq_off, counts, code, n_applied, new_len, rq_merged, qual_merged, keep=None):
        self.seq_off, self.counts, self.code, self.n_applied, self.new_len, self.rq_merged, self.qual_merged = seq_off, counts, code, n_applied, new_len, rq_merged, qual_merged
        self._keep = keep

    @classmethod
    def allocate(cls, batch: "Batch", qual_merged: bool = True, pinned: bool = False) -> "RefineReport":
        n = batch.n_zmw
        off = np.zeros(n + 1, np.int64)
        cb = batch.c_struct()
        cap = lib().ccsx_result_layout(C.byref(cb), _ptr(off, C.c_int64))
        keep = []

        def z(count, dt):
            if pinned:
                a = _pinned_array(int(count), dt, keep)
                a[...] = 0
                return a
            return np.zeros(count, dt)
        return cls(off, z(3, np.int32), z(n, np.int32), z(n, np.int32), z(n, np.int32), z(n, np.float32), z(cap, np.uint8) if qual_merged else None, keep)

    def c_struct(self) -> CRefineReport:
        c = CRefineReport()
        c.counts, c.code, c.n_applied, c.new_len = (_ptr(getattr(self, k), C.c_int32) for k in self.FIELDS[:4])
        c.rq_merged = _ptr(self.rq_merged, C.c_float)
        c.qual_merged = _ptr(self.qual_merged, C.c_uint8) if self.qual_merged is not None else None
        return c

    def quals(self, z: int) -> np.ndarray:
        """the merged quals of ZMW z"""
        o = int(self.seq_off[z])
        return self.qual_merged[o:o + int(self.new_len[z])]


# ---- pass orientation (include/ccsx.h ccsx_orient_*; DESIGN.md §2 "Pass orientation")
PASS_STRAND_UNKNOWN = 0x8    # flags bit 3: bit 0 of this pass is a guess; k_orient decides it against the ZMW's anchor pass
ORIENT_GIVEN, ORIENT_ANCHOR, ORIENT_SAME, ORIENT_OPPOSITE, ORIENT_UNDETERMINED, ORIENT_NO_ANCHOR = range(6)
ORIENT_CALL_NAMES = ["GIVEN", "ANCHOR", "SAME", "OPPOSITE", "UNDETERMINED", "NO_ANCHOR"]


class OrientOpts(C.Structure):
    _fields_ = [("min_votes", C.c_int32), ("ratio", C.c_int32)]


class COrientReport(C.Structure):
    _fields_ = [("n_reads", C.c_int32), ("strand", C.POINTER(C.c_uint8)), ("call", C.POINTER(C.c_uint8)), ("votes_same", C.POINTER(C.c_int32)),
                ("votes_opp", C.POINTER(C.c_int32))]


def orient_opts_default() -> OrientOpts:
    o = OrientOpts()
    lib().ccsx_orient_opts_default(C.byref(o))
    return o


class OrientReport:
    """ccsx_orient_report: per pass the resolved strand bit, the call (ORIENT_*) and the two vote counts."""
    FIELDS = ("strand", "call", "votes_same", "votes_opp")

    def __init__(self, strand, call, votes_same, votes_opp):
        self.strand, self.call, self.votes_same, self.votes_opp = strand, call, votes_same, votes_opp

    @classmethod
    def allocate(cls, n_reads: int) -> "OrientReport":
        return cls(np.zeros(n_reads, np.uint8), np.zeros(n_reads, np.uint8), np.zeros(n_reads, np.int32), np.zeros(n_reads, np.int32))

    def c_struct(self) -> COrientReport:
        return COrientReport(len(self.strand), _ptr(self.strand, C.c_uint8), _ptr(self.call, C.c_uint8), _ptr(self.votes_same, C.c_int32),
                             _ptr(self.votes_opp, C.c_int32))


# ---- the analyses on final reads (barcode calls, segmentation, cDNA reads): what they share.  Each supplies a set (a _PatternSet), an opts struct and a report class that
# names its request struct, its opts default and its ccsx_*_reads symbol (REQUEST, OPTS_DEFAULT, READS)
class _PatternSet:
    """a set struct of the C ABI: a count, len[max] and seq[max][max_len].  COUNT: the count's field; NOUN: what a message calls a pattern"""

    @classmethod
    def from_strings(cls, seqs):
        """from ACGT strings (either case) or arrays of codes; lengths, codes and the count are checked by the call that takes the set"""
        seqs = list(seqs)
        max_n = cls.len.size // 4
        max_len = cls.seq.size // max_n
        if len(seqs) > max_n:
            raise ValueError(f"at most {max_n} {cls.NOUN}s")
        s = cls()
        setattr(s, cls.COUNT, len(seqs))
        flat = np.frombuffer(s, np.uint8, max_n * max_len, cls.seq.offset).reshape(max_n, max_len)
        for k, q in enumerate(seqs):
            codes = ["ACGT".index(c) for c in q.upper()] if isinstance(q, str) else [int(c) for c in q]
            if len(codes) > max_len:
                raise ValueError(f"{cls.NOUN} {k}: more than {max_len} bases")
            s.len[k] = len(codes)
            flat[k, : len(codes)] = codes
        return s

    from_codes = from_strings

    def codes(self) -> list:
        return [np.array(self.seq[k][: self.len[k]], np.uint8) for k in range(getattr(self, self.COUNT))]


def _pattern_request(rep_cls, pset, opts, crep):
    """the request struct of rep_cls's analysis: (struct, what must outlive it)"""
    o = opts if opts is not None else rep_cls.OPTS_DEFAULT()
    return rep_cls.REQUEST(C.pointer(o), C.pointer(pset), C.pointer(crep), (C.c_int32 * 2)(0, 0)), (pset, o, crep)


def _reads_args(rep_cls, pset, opts, reads, report):
    """the arguments of ccsx_*_reads[_host] of rep_cls's analysis for a list of code arrays: (args, report, keep)"""
    reads = [np.ascontiguousarray(r, np.uint8) for r in reads]
    n = len(reads)
    seq_len = np.array([len(r) for r in reads], np.int32).reshape(n)
    seq_off = np.zeros(n, np.int64)
    if n:
        seq_off[1:] = np.cumsum(seq_len[:-1], dtype=np.int64)
    seq = np.concatenate(reads + [np.zeros(1, np.uint8)])
    rep = report if report is not None else rep_cls.allocate(n)
    crep = rep.c_struct()
    o = opts if opts is not None else rep_cls.OPTS_DEFAULT()
    keep = (pset, o, seq, seq_off, seq_len, crep, rep)
    return (C.byref(pset), C.byref(o), _ptr(seq, C.c_uint8), _ptr(seq_off, C.c_int64), _ptr(seq_len, C.c_int32), n, C.byref(crep)), rep, keep


def _reads_host(rep_cls, pset, reads, opts, report):
    args, rep, _keep = _reads_args(rep_cls, pset, opts, reads, report)
    name = rep_cls.READS + "_host"
    if getattr(lib(), name)(*args) != 0:
        raise RuntimeError(name + " failed: " + lib().ccsx_last_error().decode())
    return rep


# ---- barcode calls (include/ccsx.h ccsx_barcode_*; DESIGN.md §2 "Barcode calls")
BARCODE_MAX, BARCODE_MIN_LEN, BARCODE_MAX_LEN, BARCODE_MAX_WINDOW = 384, 8, 64, 1024
BARCODE_HEAD, BARCODE_TAIL = 1, 2                # the bits of BarcodeReport.call


class BarcodeOpts(C.Structure):
    _fields_ = [("window", C.c_int32), ("max_dist_pct", C.c_int32), ("min_margin", C.c_int32)]


class BarcodeSet(_PatternSet, C.Structure):
    """ccsx_barcode_set: up to 384 barcodes of 8 .. 64 codes 0 .. 3.  The barcode at a read's tail is looked for on the reverse complement of the read"""
    _fields_ = [("n_barcodes", C.c_int32), ("len", C.c_int32 * BARCODE_MAX), ("seq", (C.c_uint8 * BARCODE_MAX_LEN) * BARCODE_MAX)]
    COUNT, NOUN = "n_barcodes", "barcode"


class CBarcodeReport(C.Structure):
    _fields_ = [("n_zmw", C.c_int32)] + [(k, C.POINTER(C.c_int32)) for k in ("tested", "call", "bq", "idx", "dist", "second", "clip")]


class CBarcodeRequest(C.Structure):
    """ccsx_barcode_request: barcode calls in the fused path (ccsx_consensus_barcodes / ccsx_submit_barcodes)"""
    _fields_ = [("opts", C.POINTER(BarcodeOpts)), ("set", C.POINTER(BarcodeSet)), ("report", C.POINTER(CBarcodeReport)), ("reserved", C.c_int32 * 2)]


def barcode_opts_default() -> BarcodeOpts:
    o = BarcodeOpts()
    lib().ccsx_barcode_opts_default(C.byref(o))
    return o


class BarcodeReport(_PlaneReport):
    """ccsx_barcode_report: per read tested (0 / 1), call (BARCODE_HEAD | BARCODE_TAIL) and bq, and per end [n, 2] the best barcode, its distance, the runner-up's
    distance and the clip"""
    FIELDS = ("tested", "call", "bq", "idx", "dist", "second", "clip")
    PLANES = _int_planes("tested", "call", "bq") + tuple((k, np.int32, (2,)) for k in ("idx", "dist", "second", "clip"))
    CSTRUCT, REQUEST, OPTS_DEFAULT, READS = CBarcodeReport, CBarcodeRequest, staticmethod(barcode_opts_default), "ccsx_barcode_reads"

    def c_struct(self) -> CBarcodeReport:
        r = CBarcodeReport()
        r.n_zmw = len(self.tested)
        for k in self.FIELDS:
            setattr(r, k, _ptr(getattr(self, k), C.c_int32))
        return r

    def fields(self, z: int) -> dict:
        return {k: getattr(self, k)[z].tolist() for k in self.FIELDS}


def barcode_reads_host(bset: BarcodeSet, reads, opts: "BarcodeOpts | None" = None, report: "BarcodeReport | None" = None) -> BarcodeReport:
    """ccsx_barcode_reads_host: the barcode rule on the calling thread, no device.  reads: a list of arrays of codes 0 .. 3 (an empty one is untested)"""
    return _reads_host(BarcodeReport, bset, reads, opts, report)


# ---- segmentation of concatenated-array reads (include/ccsx.h ccsx_segment_*; DESIGN.md §2 "Segment rule")
SEGMENT_MAX_ADAPTERS, SEGMENT_MIN_LEN, SEGMENT_MAX_LEN, SEGMENT_MAX_HITS, SEGMENT_MAX_PIECES = 33, 8, 64, 64, 64
SEGMENT_PIECE_DTYPE = np.dtype([("start", np.int32), ("end", np.int32), ("index", np.uint8), ("reverse", np.uint8), ("dist_left", np.uint8),
                                ("dist_right", np.uint8)])


class SegmentOpts(C.Structure):
    _fields_ = [("max_dist_pct", C.c_int32), ("min_len", C.c_int32)]


class SegmentSet(_PatternSet, C.Structure):
    """ccsx_segment_set: the 2 .. 33 adapters of an array, of 8 .. 64 codes 0 .. 3, in array order"""
    _fields_ = [("n_adapters", C.c_int32), ("len", C.c_int32 * SEGMENT_MAX_ADAPTERS), ("seq", (C.c_uint8 * SEGMENT_MAX_LEN) * SEGMENT_MAX_ADAPTERS)]
    COUNT, NOUN = "n_adapters", "adapter"


class CSegmentPiece(C.Structure):
    _fields_ = [("start", C.c_int32), ("end", C.c_int32), ("index", C.c_uint8), ("reverse", C.c_uint8), ("dist_left", C.c_uint8), ("dist_right", C.c_uint8)]


SEGMENT_PLANES = ("tested", "overflow", "n_hits", "n_cuts", "n_segments", "complete", "orient", "leftover_bases")


class CSegmentReport(C.Structure):
    _fields_ = [("n_zmw", C.c_int32)] + [(k, C.POINTER(C.c_int32)) for k in SEGMENT_PLANES] + [("pieces", C.POINTER(CSegmentPiece))]


class CSegmentRequest(C.Structure):
    """ccsx_segment_request: segmentation in the fused path (ccsx_consensus_segments / ccsx_submit_segments)"""
    _fields_ = [("opts", C.POINTER(SegmentOpts)), ("set", C.POINTER(SegmentSet)), ("report", C.POINTER(CSegmentReport)), ("reserved", C.c_int32 * 2)]


def segment_opts_default() -> SegmentOpts:
    o = SegmentOpts()
    lib().ccsx_segment_opts_default(C.byref(o))
    return o


class SegmentReport(_PlaneReport):
    """ccsx_segment_report: per read the eight int32 planes of SEGMENT_PLANES and pieces, [n, SEGMENT_MAX_PIECES] of SEGMENT_PIECE_DTYPE: the segments by
    increasing start, zero beyond n_segments"""
    FIELDS = SEGMENT_PLANES + ("pieces",)
    PLANES = _int_planes(*SEGMENT_PLANES) + (("pieces", SEGMENT_PIECE_DTYPE, (SEGMENT_MAX_PIECES,)),)
    CSTRUCT, REQUEST, OPTS_DEFAULT, READS = CSegmentReport, CSegmentRequest, staticmethod(segment_opts_default), "ccsx_segment_reads"

    def c_struct(self) -> CSegmentReport:
        r = CSegmentReport()
        r.n_zmw = len(self.tested)
        for k in SEGMENT_PLANES:
            setattr(r, k, _ptr(getattr(self, k), C.c_int32))
        r.pieces = self.pieces.ctypes.data_as(C.POINTER(CSegmentPiece))
        return r

    def segments(self, z: int) -> list:
        """read z's segments as tuples (start, end, index, reverse, dist_left, dist_right)"""
        return [tuple(int(v) for v in p) for p in self.pieces[z, : int(self.n_segments[z])]]

    def fields(self, z: int) -> dict:
        """every plane of read z, and all SEGMENT_MAX_PIECES list entries"""
        d = {k: int(getattr(self, k)[z]) for k in SEGMENT_PLANES}
        d["pieces"] = [tuple(int(v) for v in p) for p in self.pieces[z]]
        return d


# the arguments of one analysis' read calls under their earlier names (the tests of the argument checks build their calls from them)
def _barcode_reads_args(bset, opts, reads, report):
    return _reads_args(BarcodeReport, bset, opts, reads, report)


def _segment_reads_args(sset, opts, reads, report):
    return _reads_args(SegmentReport, sset, opts, reads, report)


def segment_reads_host(sset: SegmentSet, reads, opts: "SegmentOpts | None" = None, report: "SegmentReport | None" = None) -> SegmentReport:
    """ccsx_segment_reads_host: the segment rule on the calling thread, no device.  reads: a list of arrays of codes 0 .. 3 (an empty one is untested)"""
    return _reads_host(SegmentReport, sset, reads, opts, report)


# ---- full-length cDNA reads (include/ccsx.h ccsx_cdna_*; DESIGN.md §2 "cDNA rule")
CDNA_MAX_PRIMERS, CDNA_MIN_LEN, CDNA_MAX_LEN = 64, 8, 64
CDNA_NO_PRIMER, CDNA_ONE_END, CDNA_SAME_ROLE, CDNA_SHORT, CDNA_CONCATEMER, CDNA_NO_TAIL, CDNA_FULL_LENGTH = range(7)
CDNA_NAMES = ("NO_PRIMER", "ONE_END", "SAME_ROLE", "SHORT", "CONCATEMER", "NO_TAIL", "FULL_LENGTH")
CDNA_5P, CDNA_3P = 0, 1                          # the roles of CdnaPrimers.role


class CdnaOpts(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("window", "max_dist_pct", "min_margin", "polya_mismatch", "polya_xdrop", "polya_max", "min_polya", "min_len")]


class CdnaPrimers(_PatternSet, C.Structure):
    """ccsx_cdna_set: 2 .. 64 primers of 8 .. 64 codes 0 .. 3, as the oligos, each with a role (CDNA_5P / CDNA_3P); at least one of each role"""
    _fields_ = [("n_primers", C.c_int32), ("len", C.c_int32 * CDNA_MAX_PRIMERS), ("role", C.c_uint8 * CDNA_MAX_PRIMERS),
                ("seq", (C.c_uint8 * CDNA_MAX_LEN) * CDNA_MAX_PRIMERS)]
    COUNT, NOUN = "n_primers", "primer"

    @classmethod
    def from_strings(cls, seqs, roles):
        """as _PatternSet.from_strings, with one role per primer; roles are checked by the call that takes the set"""
        seqs, roles = list(seqs), [int(r) for r in roles]
        if len(seqs) != len(roles):
            raise ValueError("one role per primer")
        s = super().from_strings(seqs)
        for k, r in enumerate(roles):
            s.role[k] = r & 0xff
        return s

    from_codes = from_strings

    def roles(self) -> list:
        return [int(self.role[k]) for k in range(self.n_primers)]


CDNA_READ_PLANES = ("tested", "cls", "strand", "start", "end", "polya_len", "n_internal", "first_internal")
CDNA_END_PLANES = ("idx", "dist", "second", "clip")


class CCdnaReport(C.Structure):
    _fields_ = [("n_zmw", C.c_int32)] + [(k, C.POINTER(C.c_int32)) for k in CDNA_READ_PLANES + CDNA_END_PLANES]


class CCdnaRequest(C.Structure):
    """ccsx_cdna_request: full-length cDNA reads in the fused path (ccsx_consensus_cdna / ccsx_submit_cdna)"""
    _fields_ = [("opts", C.POINTER(CdnaOpts)), ("set", C.POINTER(CdnaPrimers)), ("report", C.POINTER(CCdnaReport)), ("reserved", C.c_int32 * 2)]


def cdna_opts_default() -> CdnaOpts:
    o = CdnaOpts()
    lib().ccsx_cdna_opts_default(C.byref(o))
    return o


class CdnaReport(_PlaneReport):
    """ccsx_cdna_report: per read the eight int32 planes of CDNA_READ_PLANES (cls: CDNA_NAMES; the slice [start, end) of classes CONCATEMER .. FULL_LENGTH) and
    per end [n, 2] the best primer, its distance, the runner-up's distance and the clip"""
    FIELDS = CDNA_READ_PLANES + CDNA_END_PLANES
    PLANES = _int_planes(*CDNA_READ_PLANES) + tuple((k, np.int32, (2,)) for k in CDNA_END_PLANES)
    CSTRUCT, REQUEST, OPTS_DEFAULT, READS = CCdnaReport, CCdnaRequest, staticmethod(cdna_opts_default), "ccsx_cdna_reads"

    def c_struct(self) -> CCdnaReport:
        r = CCdnaReport()
        r.n_zmw = len(self.tested)
        for k in self.FIELDS:
            setattr(r, k, _ptr(getattr(self, k), C.c_int32))
        return r

    def fields(self, z: int) -> dict:
        return {k: getattr(self, k)[z].tolist() for k in self.FIELDS}


def cdna_reads_host(primers: CdnaPrimers, reads, opts: "CdnaOpts | None" = None, report: "CdnaReport | None" = None) -> CdnaReport:
    """ccsx_cdna_reads_host: the cDNA rule on the calling thread, no device.  reads: a list of arrays of codes 0 .. 3 (an empty one is untested)"""
    return _reads_host(CdnaReport, primers, reads, opts, report)


# ---- cell barcodes and UMIs (include/ccsx.h ccsx_cell_*; DESIGN.md §2 "Cell-tag rule")
CELL_MAX_FIELD, CELL_MAX_WHITELIST = 16, 1 << 23
CELL_NONE, CELL_RAW, CELL_EXACT, CELL_CORRECTED, CELL_AMBIGUOUS, CELL_ABSENT = range(6)
CELL_NAMES = ("NONE", "RAW", "EXACT", "CORRECTED", "AMBIGUOUS", "ABSENT")
CELL_PLANES = ("tag", "bc_raw", "bc", "bc_hi", "kind", "shift", "umi", "tag_clip")
_CELL_UNSIGNED = ("bc_raw", "umi")


class CellDesign(C.Structure):
    """ccsx_cell_design: umi_len and bc_len (0 .. 16, at least one base together), side (0: at the 5' primer, 1: at the 3' primer), bc_first (1: the barcode is
    next to the primer), indels (1: candidates with a lost or a gained base are tried)"""
    _fields_ = [(k, C.c_int32) for k in ("umi_len", "bc_len", "side", "bc_first", "indels")] + [("reserved", C.c_int32 * 3)]

    @classmethod
    def default(cls) -> "CellDesign":
        d = cls()
        lib().ccsx_cell_design_default(C.byref(d))
        return d


class CCellReport(C.Structure):
    _fields_ = [("cdna", CCdnaReport)] + [(k, C.POINTER(C.c_uint32 if k in _CELL_UNSIGNED else C.c_int32)) for k in CELL_PLANES]


class CellWhitelist:
    """ccsx_cell_whitelist: owns the host object and frees it.  barcodes: ACGT strings (either case) or arrays of codes, all of bc_len bases"""

    def __init__(self, barcodes, bc_len: "int | None" = None):
        if isinstance(barcodes, np.ndarray) and barcodes.ndim == 2:   # [n, bc_len] codes as they are
            rows, self.bc_len = barcodes, int(barcodes.shape[1])
        else:
            rows = [["ACGT".index(c) for c in q.upper()] if isinstance(q, str) else [int(c) for c in q] for q in barcodes]
            self.bc_len = int(bc_len) if bc_len is not None else (len(rows[0]) if rows else 0)
            if any(len(r) != self.bc_len for r in rows):
                raise ValueError(f"every barcode of a whitelist has bc_len = {self.bc_len} bases")
        codes = np.ascontiguousarray(np.array(rows, np.uint8).reshape(len(rows), self.bc_len))
        self.n = len(rows)
        self._p = lib().ccsx_cell_whitelist_create(_ptr(codes, C.c_uint8) if codes.size else None, self.n, self.bc_len)
        if not self._p:
            raise RuntimeError("ccsx_cell_whitelist_create failed: " + lib().ccsx_last_error().decode())

    @property
    def table(self) -> np.ndarray:
        """a copy of the table's uint64 slots"""
        slots, tab = C.c_uint32(0), C.POINTER(C.c_uint64)()
        lib().ccsx_cell_whitelist_info(self._p, None, None, C.byref(slots), C.byref(tab))
        return np.ctypeslib.as_array(tab, (slots.value,)).copy()

    def close(self):
        if getattr(self, "_p", None):
            lib().ccsx_cell_whitelist_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cell_slot(key: int, slots: int) -> int:
    """ccsx_cell_slot: the first slot of key in a table of `slots` slots"""
    return int(lib().ccsx_cell_slot(key & 0xffffffff, slots))


class CellReport(_PlaneReport):
    """ccsx_cell_report: the planes of CdnaReport (clip: the primers' own) and per read the eight planes of CELL_PLANES (tag: CELL_NAMES; bc_raw and umi uint32)"""
    FIELDS = CdnaReport.FIELDS + CELL_PLANES
    PLANES = CdnaReport.PLANES + tuple((k, np.uint32 if k in _CELL_UNSIGNED else np.int32, ()) for k in CELL_PLANES)
    CSTRUCT = CCellReport

    def c_struct(self) -> CCellReport:
        r = CCellReport()
        r.cdna.n_zmw = len(self.tested)
        for k in CdnaReport.FIELDS:
            setattr(r.cdna, k, _ptr(getattr(self, k), C.c_int32))
        for k in CELL_PLANES:
            setattr(r, k, _ptr(getattr(self, k), C.c_uint32 if k in _CELL_UNSIGNED else C.c_int32))
        return r

    def fields(self, z: int) -> dict:
        return {k: getattr(self, k)[z].tolist() for k in self.FIELDS}


def _cell_reads_args(primers, opts, design, whitelist, reads, report):
    """the arguments of ccsx_cell_reads[_host] for a list of code arrays: (args, report, keep)"""
    (pset, o, seq, off, ln, n, crep), rep, keep = _reads_args(CellReport, primers, opts if opts is not None else cdna_opts_default(), reads, report)
    d = design if design is not None else CellDesign.default()
    return (pset, o, C.byref(d), whitelist._p if whitelist is not None else None, seq, off, ln, n, crep), rep, keep + (d, whitelist)


def cell_reads_host(primers: CdnaPrimers, reads, design: "CellDesign | None" = None, whitelist: "CellWhitelist | None" = None, opts: "CdnaOpts | None" = None,
                    report: "CellReport | None" = None) -> CellReport:
    """ccsx_cell_reads_host: the cell-tag rule on the calling thread, no device.  reads: a list of arrays of codes 0 .. 3 (an empty one is untested)"""
    args, rep, _keep = _cell_reads_args(primers, opts, design, whitelist, reads, report)
    if lib().ccsx_cell_reads_host(*args) != 0:
        raise RuntimeError("ccsx_cell_reads_host failed: " + lib().ccsx_last_error().decode())
    return rep


# ---- duplicate reads (include/ccsx.h ccsx_dup_*; DESIGN.md §2 "Duplicate rule")
DUP_MAX_BUCKET, DUP_MAX_READS = 512, 1 << 24
DUP_UNTESTED, DUP_TESTED, DUP_OVERFLOW = 0, 1, 2
DUP_SIG_DTYPE = np.dtype([("end", np.uint64, (2, 2)), ("mini", np.uint32, (2,)), ("len", np.int32), ("window", np.int32)])   # ccsx_dup_sig, 48 bytes


class DupOpts(C.Structure):
    _fields_ = [("window", C.c_int32), ("kmer", C.c_int32), ("max_dist_pct", C.c_int32), ("max_len_diff_pct", C.c_int32)]


class CDupReport(C.Structure):
    _fields_ = [("n", C.c_int32)] + [(k, C.POINTER(C.c_int32)) for k in ("status", "rep", "set_size", "dup")]


def dup_opts_default() -> DupOpts:
    o = DupOpts()
    lib().ccsx_dup_opts_default(C.byref(o))
    return o


class DupReport(_PlaneReport):
    """ccsx_dup_report: per read status (DUP_UNTESTED / DUP_TESTED / DUP_OVERFLOW), rep (the representative of its set), set_size and dup (0 / 1)"""
    FIELDS = ("status", "rep", "set_size", "dup")
    PLANES = _int_planes(*FIELDS)
    CSTRUCT = CDupReport

    def c_struct(self) -> CDupReport:
        r = CDupReport()
        r.n = len(self.status)
        for k in self.FIELDS:
            setattr(r, k, _ptr(getattr(self, k), C.c_int32))
        return r

    def fields(self, z: int) -> dict:
        return {k: int(getattr(self, k)[z]) for k in self.FIELDS}


def _dup_sign_args(reads, opts):
    """the arguments of ccsx_dup_sign_reads[_host]: (args, signatures, keep).  reads: a list of code arrays, or the tuple (seq, seq_off, seq_len) of the C call"""
    if isinstance(reads, tuple):
        seq, seq_off, seq_len = (np.ascontiguousarray(a, t) for a, t in zip(reads, (np.uint8, np.int64, np.int32)))
        n = len(seq_len)
    else:
        reads = [np.ascontiguousarray(r, np.uint8) for r in reads]
        n = len(reads)
        seq_len = np.array([len(r) for r in reads], np.int32).reshape(n)
        seq_off = np.zeros(n, np.int64)
        if n:
            seq_off[1:] = np.cumsum(seq_len[:-1], dtype=np.int64)
        seq = np.concatenate(reads + [np.zeros(1, np.uint8)])
    sig = np.zeros(n, DUP_SIG_DTYPE)
    o = opts if opts is not None else dup_opts_default()
    return (C.byref(o), _ptr(seq, C.c_uint8), _ptr(seq_off, C.c_int64), _ptr(seq_len, C.c_int32), n, sig.ctypes.data_as(C.c_void_p)), sig, (o, seq, seq_off, seq_len)


def _dup_cluster_args(sig, group, score, opts, report):
    """the arguments of ccsx_dup_cluster[_host]: (args, report, keep).  group / score: None (all 0) or one int32 per read"""
    sig = np.ascontiguousarray(sig, DUP_SIG_DTYPE)
    n = len(sig)
    g = None if group is None else np.ascontiguousarray(group, np.int32).reshape(n)
    sc = None if score is None else np.ascontiguousarray(score, np.int32).reshape(n)
    rep = report if report is not None else DupReport.allocate(n)
    crep = rep.c_struct()
    o = opts if opts is not None else dup_opts_default()
    null = C.POINTER(C.c_int32)()
    return (C.byref(o), sig.ctypes.data_as(C.c_void_p), null if g is None else _ptr(g, C.c_int32), null if sc is None else _ptr(sc, C.c_int32), n,
            C.byref(crep)), rep, (o, sig, g, sc, crep)


def dup_sign_host(reads, opts: "DupOpts | None" = None) -> np.ndarray:
    """ccsx_dup_sign_reads_host: the signatures (DUP_SIG_DTYPE) of a list of arrays of codes 0 .. 3 on the calling thread, no device"""
    args, sig, _keep = _dup_sign_args(reads, opts)
    if lib().ccsx_dup_sign_reads_host(*args) != 0:
        raise RuntimeError("ccsx_dup_sign_reads_host failed: " + lib().ccsx_last_error().decode())
    return sig


def dup_cluster_host(sig, group=None, score=None, opts: "DupOpts | None" = None, report: "DupReport | None" = None) -> DupReport:
    """ccsx_dup_cluster_host: the duplicate sets of the signatures on the calling thread, no device"""
    args, rep, _keep = _dup_cluster_args(sig, group, score, opts, report)
    if lib().ccsx_dup_cluster_host(*args) != 0:
        raise RuntimeError("ccsx_dup_cluster_host failed: " + lib().ccsx_last_error().decode())
    return rep


# ---- representative reads (include/ccsx.h ccsx_represent_*; DESIGN.md §2 "Representative rule")
REPRESENT_POLISHED, REPRESENT_NONE, REPRESENT_DRAFT, REPRESENT_SUBREAD = 0, 1, 2, 3
REPRESENT_NAMES = ("POLISHED", "NONE", "DRAFT", "SUBREAD")
REPRESENT_QV = 10                                # qual / raw_qv of every base of an unpolished representative


class CRepresentReport(C.Structure):
    _fields_ = [("n_zmw", C.c_int32), ("cls", C.POINTER(C.c_int32)), ("pass", C.POINTER(C.c_int32))]


class CRepresentRequest(C.Structure):
    """ccsx_represent_request: representative reads in the fused path (ccsx_consensus_represent / ccsx_submit_represent)"""
    _fields_ = [("subread_fallback", C.c_int32), ("kinetics", C.c_int32), ("report", C.POINTER(CRepresentReport)), ("reserved", C.c_int32 * 2)]


class RepresentReport(_PlaneReport):
    """ccsx_represent_report: per ZMW cls (REPRESENT_*) and pass_ (SUBREAD: the representative pass, index within the ZMW; else -1)"""
    PLANES = _int_planes("cls", "pass_")
    CSTRUCT = CRepresentReport

    def c_struct(self) -> CRepresentReport:
        r = CRepresentReport()
        r.n_zmw = len(self.cls)
        r.cls = _ptr(self.cls, C.c_int32)
        setattr(r, "pass", _ptr(self.pass_, C.c_int32))
        return r


def _represent_request(report: RepresentReport, subread_fallback, kinetics):
    crep = report.c_struct()
    return CRepresentRequest(int(subread_fallback), int(kinetics), C.pointer(crep), (C.c_int32 * 2)(0, 0)), (crep, report)


def represent_host(batch: "Batch", opts: "Opts", status, drafts, res: "Results", subread_fallback=False, kinetics=False,
                   report: "RepresentReport | None" = None) -> RepresentReport:
    """ccsx_represent_host: the representative rule on the calling thread, no device, applied in place to `res` (the Results of a finished run on `batch`, or
    planes of the caller's making on the capacity layout).  status: [n_zmw] the final statuses; drafts: one array of codes per ZMW (an empty one: no draft)"""
    n = batch.n_zmw
    drafts = [np.ascontiguousarray(d, np.uint8) for d in drafts]
    if len(drafts) != n:
        raise ValueError("drafts: one array per ZMW")
    st = np.ascontiguousarray(status, np.int32)
    dlen = np.array([len(d) for d in drafts], np.int32).reshape(n)
    doff = np.zeros(n, np.int64)
    if n:
        doff[1:] = np.cumsum(dlen[:-1], dtype=np.int64)
    dseq = np.concatenate(drafts + [np.zeros(1, np.uint8)])
    rep = report if report is not None else RepresentReport.allocate(n)
    req, _keep = _represent_request(rep, subread_fallback, kinetics)
    cb, cr = batch.c_struct(), res.c_struct()
    if lib().ccsx_represent_host(C.byref(cb), C.byref(opts), _ptr(st, C.c_int32), _ptr(dseq, C.c_uint8), _ptr(doff, C.c_int64), _ptr(dlen, C.c_int32),
                                 C.byref(req), C.byref(cr)) != 0:
        raise RuntimeError("ccsx_represent_host failed: " + lib().ccsx_last_error().decode())
    return rep


class CPileup(C.Structure):
    _fields_ = [("seq_capacity", C.c_int64), ("coverage", C.POINTER(C.c_uint8)), ("matches", C.POINTER(C.c_uint8)),
                ("mismatches", C.POINTER(C.c_uint8))]


@dataclass
class Pileup:
    """ccsx_pileup: the per-base pileup summary (DESIGN.md §2 "Pileup summary"), planes indexed like Results.seq.  sa / sm / sx give one ZMW's
    tags of docs/faq/bam-output.md:25-27: sa run-length encoded as uint32 (length, coverage) pairs, sm / sx as uint8 per base."""
    seq_off: np.ndarray
    seq_len: np.ndarray
    coverage: np.ndarray
    matches: np.ndarray
    mismatches: np.ndarray

    @staticmethod
    def allocate(results: "Results", pinned: bool = False) -> "Pileup":
        """three planes of the results' capacity; seq_off / seq_len are the results' own arrays (filled when the results are).  pinned=True: page-locked
        planes for Handle.submit"""
        cap = len(results.seq)
        keep = []

        def z():
            if not pinned:
                return np.zeros(cap, np.uint8)
            p = lib().ccsx_alloc_pinned(max(1, cap))
            if not p:
                raise RuntimeError("ccsx_alloc_pinned failed: " + lib().ccsx_last_error().decode())
            keep.append(_Pinned(p))
            a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(max(1, cap),))[:cap]
            a[...] = 0
            return a
        pl = Pileup(results.seq_off, results.seq_len, z(), z(), z())
        pl._pinned = keep
        return pl

    def c_struct(self) -> CPileup:
        c = CPileup()
        c.seq_capacity = len(self.coverage)
        c.coverage, c.matches, c.mismatches = (_ptr(a, C.c_uint8) for a in (self.coverage, self.matches, self.mismatches))
        return c

    def _plane(self, a: np.ndarray, z: int) -> np.ndarray:
        o = int(self.seq_off[z])
        return a[o:o + int(self.seq_len[z])]

    def cov(self, z: int) -> np.ndarray:
        return self._plane(self.coverage, z)

    def sm(self, z: int) -> np.ndarray:
        return self._plane(self.matches, z)

    def sx(self, z: int) -> np.ndarray:
        return self._plane(self.mismatches, z)

    def sa(self, z: int) -> np.ndarray:
        return rle(self.cov(z))


def rle(v: np.ndarray) -> np.ndarray:
    """run-length encoding of a plane as the sa tag stores it: uint32 [length, value, length, value, ...]"""
    v = np.asarray(v)
    if len(v) == 0:
        return np.zeros(0, np.uint32)
    starts = np.flatnonzero(np.concatenate([[True], v[1:] != v[:-1]]))
    lens = np.diff(np.concatenate([starts, [len(v)]]))
    return np.stack([lens, v[starts]], axis=1).astype(np.uint32).reshape(-1)


def unrle(pairs: np.ndarray) -> np.ndarray:
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    return np.repeat(p[:, 1], p[:, 0]).astype(np.uint8)


class CExtras(C.Structure):
    """ccsx_extras: optional outputs of the fused path (include/ccsx.h)"""
    _fields_ = [("pile", C.POINTER(CPileup)), ("tandem_len", C.POINTER(C.c_int32)), ("min_tandem_repeat_length", C.c_int32), ("reserved", C.c_int32)]


class CRequests(C.Structure):
    """ccsx_requests: every optional request of the fused path (ccsx_consensus_requests / ccsx_submit_requests); any member may be NULL"""
    _fields_ = [("ex", C.POINTER(CExtras)), ("fold", C.POINTER(CFoldRequest)), ("adapters", C.POINTER(CAdapterRequest)), ("control", C.POINTER(CControlRequest)),
                ("coverage", C.POINTER(CCoverageRequest)), ("reserved", C.c_void_p * 3)]


def tandem_buffer(n_zmw: int, pinned: bool = False) -> np.ndarray:
    """an int32 [n_zmw] destination for tandem_len; pinned=True: page-locked (Handle.submit), kept alive by the array"""
    if not pinned:
        return np.zeros(n_zmw, np.int32)
    p = lib().ccsx_alloc_pinned(max(1, n_zmw) * 4)
    if not p:
        raise RuntimeError("ccsx_alloc_pinned failed: " + lib().ccsx_last_error().decode())
    owner = _Pinned(p)
    a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int32)), shape=(max(1, n_zmw),))[:n_zmw]
    a[...] = 0
    _PINNED_OWNERS[id(a)] = owner   # the page-locked block is freed with the array
    weakref.finalize(a, _PINNED_OWNERS.pop, id(a), None)
    return a


_PINNED_OWNERS: dict = {}


def _pinned_array(count: int, dt, keep: list) -> np.ndarray:
    """count elements of dt in one ccsx_alloc_pinned block, owned by an entry appended to keep"""
    dt = np.dtype(dt)
    nb = max(1, int(count) * dt.itemsize)
    p = lib().ccsx_alloc_pinned(nb)
    if not p:
        raise RuntimeError("ccsx_alloc_pinned failed: " + lib().ccsx_last_error().decode())
    keep.append(_Pinned(p))
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(nb,))[: int(count) * dt.itemsize].view(dt)


class DeflateBlock(C.Structure):
    _fields_ = [("in_off", C.c_int64), ("in_len", C.c_int32), ("out_len", C.c_int32), ("out_off", C.c_int64)]


class DeflateSpan(C.Structure):
    _fields_ = [("in_off", C.c_int64), ("in_len", C.c_int32), ("out_cap", C.c_int32), ("out_off", C.c_int64)]


class Timings(C.Structure):
    _fields_ = [
        ("setup_ms", C.c_float), ("draft_ms", C.c_float), ("align_ms", C.c_float), ("polish_ms", C.c_float),
        ("stitch_ms", C.c_float), ("total_ms", C.c_float), ("polish_workgroups", C.c_int64),
        ("queue_ms", C.c_float), ("reserved_", C.c_float), ("start_ms", C.c_double), ("end_ms", C.c_double),
    ]


# ---- model training (include/ccsx.h ccsx_train_*, ccsx_fitter_*; DESIGN.md §2 "Model training")
TRAIN_FRAC = 32


class CTrainCounts(C.Structure):
    _fields_ = [("n_zmw", C.c_int32), ("reserved", C.c_int32), ("match", C.POINTER(C.c_int64)), ("stay", C.POINTER(C.c_int64)),
                ("del_", C.POINTER(C.c_int64)), ("loglik", C.POINTER(C.c_int64)), ("n_pairs", C.POINTER(C.c_int32)), ("n_gated", C.POINTER(C.c_int32)),
                ("n_bases", C.POINTER(C.c_int32)), ("status", C.POINTER(C.c_int32))]


class FitOpts(C.Structure):
    _fields_ = [("degree", C.c_int32), ("snr_bins", C.c_int32), ("min_events", C.c_double), ("pseudo", C.c_double)]


class FitReport(C.Structure):
    _fields_ = [("pairs", C.c_int64), ("gated", C.c_int64), ("bases", C.c_int64), ("loglik_per_base", C.c_double), ("contexts_kept", C.c_int32),
                ("snr_lo", C.c_float), ("snr_hi", C.c_float), ("max_change", C.c_double)]


def fit_opts_default() -> FitOpts:
    o = FitOpts()
    lib().ccsx_fit_opts_default(C.byref(o))
    return o


class TrainCounts:
    """ccsx_train_counts: per ZMW the posterior event counts x 2^32 (match, stay [n, 16, 12], del_ [n, 16]; `del` is a Python keyword), loglik x 65536,
    the pair / gated-pair / base counts and the status after the cascade."""
    PLANES = (("match", np.int64, (NCTX, NOBS)), ("stay", np.int64, (NCTX, NOBS)), ("del_", np.int64, (NCTX,)), ("loglik", np.int64, ()),
              ("n_pairs", np.int32, ()), ("n_gated", np.int32, ()), ("n_bases", np.int32, ()), ("status", np.int32, ()))

    def __init__(self, n: int):
        for k, dt, shape in self.PLANES:
            setattr(self, k, np.zeros((n,) + shape, dt))

    @classmethod
    def allocate(cls, batch: "Batch | int") -> "TrainCounts":
        return cls(batch if isinstance(batch, int) else batch.n_zmw)

    @property
    def n_zmw(self) -> int:
        return len(self.loglik)

    def c_struct(self) -> CTrainCounts:
        c = CTrainCounts()
        c.n_zmw = self.n_zmw; c.reserved = 0
        types = dict(CTrainCounts._fields_)
        for k, _, _ in self.PLANES:
            setattr(c, k, getattr(self, k).ctypes.data_as(types[k]))
        return c

    def add(self, other: "TrainCounts") -> "TrainCounts":
        """the exact int64 sum, ZMW by ZMW (the status is kept)"""
        assert other.n_zmw == self.n_zmw
        for k, _, _ in self.PLANES[:-1]:
            getattr(self, k)[...] += getattr(other, k)
        return self

    def rows(self, zs) -> "TrainCounts":
        """the ZMWs `zs`, in that order, as a new object"""
        zs = np.asarray(zs, np.int64)
        out = TrainCounts(len(zs))
        for k, _, _ in self.PLANES:
            getattr(out, k)[...] = getattr(self, k)[zs]
        return out


def train_pair_host(model: Model, snr, tpl, left_flank: int, cs: int, ce: int, obs, min_zscore: float = 0.0, out=None, J: "int | None" = None, n: "int | None" = None):
    """ccsx_train_pair_host: one pair on the host.  Returns (rc, match[16, 12], stay[16, 12], del[16], loglik[1]) — the int64 arrays of `out` (the same tuple without
    rc), which are added to, or fresh zeroed ones.  rc: 1 counted, 0 gated, < 0 bad argument.  J / n override the array lengths (argument tests)"""
    snr = np.ascontiguousarray(snr, np.float32); tpl = np.ascontiguousarray(tpl, np.uint8); obs = np.ascontiguousarray(obs, np.uint8)
    m, s, d, ll = out if out is not None else (np.zeros((NCTX, NOBS), np.int64), np.zeros((NCTX, NOBS), np.int64), np.zeros(NCTX, np.int64), np.zeros(1, np.int64))
    rc = lib().ccsx_train_pair_host(C.byref(model), _ptr(snr, C.c_float), _ptr(tpl, C.c_uint8), len(tpl) if J is None else J, int(left_flank), int(cs), int(ce),
                                    _ptr(obs, C.c_uint8), len(obs) if n is None else n, float(min_zscore), _ptr(m, C.c_int64), _ptr(s, C.c_int64),
                                    _ptr(d, C.c_int64), _ptr(ll, C.c_int64))
    return rc, m, s, d, ll


class Fitter:
    """ccsx_fitter: the M-step.  Fitter(start, opts).add(counts, snr) ... .finish() -> (Model, FitReport); host only, no device."""

    def __init__(self, start: Model, opts: "FitOpts | None" = None):
        self._L = lib()
        self._f = C.c_void_p()
        o = opts if opts is not None else fit_opts_default()
        if self._L.ccsx_fitter_create(C.byref(start), C.byref(o), C.byref(self._f)) != 0:
            raise RuntimeError("ccsx_fitter_create failed: " + self._L.ccsx_last_error().decode())

    def add(self, counts: TrainCounts, snr) -> "Fitter":
        snr = np.ascontiguousarray(snr, np.float32)
        assert snr.shape == (counts.n_zmw, 4)
        cc = counts.c_struct()
        if self._L.ccsx_fitter_add(self._f, C.byref(cc), _ptr(snr, C.c_float)) != 0:
            raise RuntimeError("ccsx_fitter_add failed: " + self._L.ccsx_last_error().decode())
        return self

    def finish(self) -> "tuple[Model, FitReport]":
        m, rep = Model(), FitReport()
        if self._L.ccsx_fitter_finish(self._f, C.byref(m), C.byref(rep)) != 0:
            raise RuntimeError("ccsx_fitter_finish failed: " + self._L.ccsx_last_error().decode())
        return m, rep

    def close(self):
        if self._f:
            self._L.ccsx_fitter_destroy(self._f)
            self._f = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CSynth(C.Structure):
    _fields_ = [("batch", CBatch), ("tpl_off", C.POINTER(C.c_int64)), ("tpl", C.POINTER(C.c_uint8))]


# every symbol include/ccsx.h declares (tests/test_abi.py checks the library exports all of them)
EXPORTS = [
    "ccsx_abi_version", "ccsx_spec_version", "ccsx_last_error", "ccsx_device_count", "ccsx_model_default", "ccsx_opts_default",
    "ccsx_create", "ccsx_destroy", "ccsx_result_layout", "ccsx_consensus_batch", "ccsx_upload", "ccsx_run",
    "ccsx_sync", "ccsx_download", "ccsx_get_timings", "ccsx_stage_draft", "ccsx_stage_align",
    "ccsx_stage_windows", "ccsx_synth_generate", "ccsx_synth_free", "ccsx_alloc_pinned", "ccsx_free_pinned",
    "ccsx_submit", "ccsx_wait", "ccsx_poll", "ccsx_ticket_timings",
    "ccsx_model_from_json", "ccsx_model_load", "ccsx_model_to_json", "ccsx_model_for_chemistry",
    "ccsx_build_flags", "ccsx_runtime_switches", "ccsx_pci_numa_node", "ccsx_device_numa_node", "ccsx_bind_thread_to_node", "ccsx_bind_thread_to_device", "ccsx_draft_layout", "ccsx_draft_batch", "ccsx_polish_batch", "ccsx_submit_draft", "ccsx_submit_polish",
    "ccsx_hd_opts_default", "ccsx_hd_rule_version", "ccsx_hd_batch",
    "ccsx_pileup_rule_version", "ccsx_consensus_pileup", "ccsx_submit_pileup", "ccsx_stage_polished", "ccsx_stage_align_ev",
    "ccsx_poa_log", "ccsx_stage_poa", "ccsx_stage_wmeta",
    "ccsx_tandem_rule_version", "ccsx_consensus_extras", "ccsx_submit_extras",
    "ccsx_consensus_hd", "ccsx_submit_hd", "ccsx_consensus_hd_requests", "ccsx_submit_hd_requests",
    "ccsx_fold_opts_default", "ccsx_fold_rule_version", "ccsx_consensus_fold", "ccsx_submit_fold",
    "ccsx_adapter_opts_default", "ccsx_adapter_rule_version", "ccsx_adapter_set_default", "ccsx_consensus_screen", "ccsx_submit_screen",
    "ccsx_control_opts_default", "ccsx_control_rule_version", "ccsx_consensus_control", "ccsx_submit_control",
    "ccsx_coverage_opts_default", "ccsx_coverage_rule_version", "ccsx_consensus_requests", "ccsx_submit_requests",
    "ccsx_orient_opts_default", "ccsx_orient_rule_version", "ccsx_orient_batch", "ccsx_set_orient_opts", "ccsx_stage_orient",
    "ccsx_handoff_opts_default", "ccsx_handoff_rule_version", "ccsx_consensus_handoff", "ccsx_submit_handoff",
    "ccsx_refine_tiles_init", "ccsx_refine_rule_version", "ccsx_refine_perr", "ccsx_refine_batch", "ccsx_submit_refine",
    "ccsx_inflate_rule_version", "ccsx_inflater_create", "ccsx_inflater_destroy", "ccsx_inflate_blocks", "ccsx_inflate_submit", "ccsx_inflate_wait",
    "ccsx_inflate_blocks_host",
    "ccsx_deflate_rule_version", "ccsx_deflate_bound", "ccsx_deflater_create", "ccsx_deflater_destroy", "ccsx_deflate_spans", "ccsx_deflate_submit",
    "ccsx_deflate_wait", "ccsx_deflate_spans_host", "ccsx_deflate_crc", "ccsx_deflate_fill_spans", "ccsx_deflate_code_lengths",
    "ccsx_train_rule_version", "ccsx_train_batch", "ccsx_train_pair_host",
    "ccsx_fit_opts_default", "ccsx_fitter_create", "ccsx_fitter_add", "ccsx_fitter_finish", "ccsx_fitter_destroy",
    "ccsx_barcode_opts_default", "ccsx_barcode_rule_version", "ccsx_barcode_reads_host", "ccsx_barcode_reads", "ccsx_consensus_barcodes", "ccsx_submit_barcodes",
    "ccsx_segment_opts_default", "ccsx_segment_rule_version", "ccsx_segment_chunk", "ccsx_segment_reads_host", "ccsx_segment_reads", "ccsx_consensus_segments",
    "ccsx_submit_segments",
    "ccsx_cdna_opts_default", "ccsx_cdna_rule_version", "ccsx_cdna_reads_host", "ccsx_cdna_reads", "ccsx_consensus_cdna", "ccsx_submit_cdna",
    "ccsx_represent_rule_version", "ccsx_represent_host", "ccsx_consensus_represent", "ccsx_submit_represent",
    "ccsx_dup_opts_default", "ccsx_dup_rule_version", "ccsx_dup_hash", "ccsx_dup_sign_reads_host", "ccsx_dup_sign_reads", "ccsx_dup_cluster_host", "ccsx_dup_cluster",
    "ccsx_cell_design_default", "ccsx_cell_rule_version", "ccsx_cell_slot", "ccsx_cell_whitelist_create", "ccsx_cell_whitelist_destroy", "ccsx_cell_whitelist_info",
    "ccsx_cell_reads_host", "ccsx_cell_reads",
]

_lib = None


def lib() -> C.CDLL:
    """Load libccsx.so (fails loudly when it has not been built: run __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built — run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(LIB_PATH)
        L.ccsx_last_error.restype = C.c_char_p
        L.ccsx_result_layout.restype = C.c_int64
        L.ccsx_result_layout.argtypes = [C.POINTER(CBatch), C.POINTER(C.c_int64)]
        L.ccsx_create.argtypes = [C.c_int, C.POINTER(Model), C.POINTER(Opts), C.POINTER(C.c_void_p)]
        for f in ("ccsx_destroy", "ccsx_run", "ccsx_sync"):
            getattr(L, f).argtypes = [C.c_void_p]
        L.ccsx_upload.argtypes = [C.c_void_p, C.POINTER(CBatch)]
        L.ccsx_download.argtypes = [C.c_void_p, C.POINTER(CResults)]
        L.ccsx_consensus_batch.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults)]
        L.ccsx_get_timings.argtypes = [C.c_void_p, C.POINTER(Timings)]
        L.ccsx_submit.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(C.c_int64)]
        L.ccsx_wait.argtypes = [C.c_void_p, C.c_int64]
        L.ccsx_poll.argtypes = [C.c_void_p, C.c_int64]
        L.ccsx_ticket_timings.argtypes = [C.c_void_p, C.c_int64, C.POINTER(Timings)]
        L.ccsx_stage_draft.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_uint8), C.c_int32, C.POINTER(C.c_int32)]
        L.ccsx_stage_align.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int32,
                                       C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.ccsx_stage_windows.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32)]
        L.ccsx_stage_align_ev.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                          C.POINTER(C.c_uint8), C.c_int32]
        L.ccsx_stage_wmeta.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32)]
        L.ccsx_poa_log.argtypes = [C.c_void_p, C.c_int32]
        L.ccsx_stage_poa.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32)]
        L.ccsx_synth_generate.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_uint64, C.POINTER(C.POINTER(CSynth))]
        L.ccsx_synth_free.argtypes = [C.POINTER(CSynth)]
        L.ccsx_alloc_pinned.restype = C.c_void_p
        L.ccsx_alloc_pinned.argtypes = [C.c_size_t]
        L.ccsx_free_pinned.argtypes = [C.c_void_p]
        L.ccsx_model_default.argtypes = [C.POINTER(Model)]
        L.ccsx_model_from_json.argtypes = [C.c_char_p, C.POINTER(Model)]
        L.ccsx_model_load.argtypes = [C.c_char_p, C.POINTER(Model)]
        L.ccsx_model_to_json.restype = C.c_int64
        L.ccsx_model_to_json.argtypes = [C.POINTER(Model), C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int64]
        L.ccsx_model_for_chemistry.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(Model)]
        L.ccsx_opts_default.argtypes = [C.POINTER(Opts)]
        L.ccsx_build_flags.restype = C.c_char_p
        L.ccsx_runtime_switches.restype = C.c_char_p
        L.ccsx_draft_layout.restype = None
        L.ccsx_draft_layout.argtypes = [C.POINTER(CBatch), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.ccsx_draft_batch.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CDrafts)]
        L.ccsx_polish_batch.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CDrafts), C.POINTER(CResults), C.c_uint32]
        L.ccsx_submit_draft.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CDrafts), C.POINTER(C.c_int64)]
        L.ccsx_submit_polish.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CDrafts), C.POINTER(CResults), C.c_uint32, C.POINTER(C.c_int64)]
        L.ccsx_hd_opts_default.restype = None
        L.ccsx_hd_opts_default.argtypes = [C.POINTER(HdOpts)]
        L.ccsx_hd_batch.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CDrafts), C.POINTER(HdOpts), C.POINTER(CHdReport)]
        L.ccsx_consensus_pileup.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(CPileup)]
        L.ccsx_submit_pileup.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(CPileup), C.POINTER(C.c_int64)]
        L.ccsx_stage_polished.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32),
                                          C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.ccsx_consensus_extras.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(CExtras)]
        L.ccsx_submit_extras.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(CExtras), C.POINTER(C.c_int64)]
        L.ccsx_consensus_hd.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(CExtras), C.POINTER(CHdRequest)]
        L.ccsx_submit_hd.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(CExtras), C.POINTER(CHdRequest), C.POINTER(C.c_int64)]
        L.ccsx_consensus_hd_requests.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(CRequests), C.POINTER(CHdRequest)]
        L.ccsx_submit_hd_requests.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(CRequests), C.POINTER(CHdRequest), C.POINTER(C.c_int64)]
        L.ccsx_fold_opts_default.restype = None
        L.ccsx_fold_opts_default.argtypes = [C.POINTER(FoldOpts)]
        L.ccsx_consensus_fold.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(CExtras), C.POINTER(CFoldRequest)]
        L.ccsx_submit_fold.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(CExtras), C.POINTER(CFoldRequest), C.POINTER(C.c_int64)]
        L.ccsx_adapter_opts_default.restype = None
        L.ccsx_adapter_opts_default.argtypes = [C.POINTER(AdapterOpts)]
        L.ccsx_adapter_set_default.argtypes = [C.POINTER(AdapterSet)]
        L.ccsx_consensus_screen.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(CExtras), C.POINTER(CFoldRequest), C.POINTER(CAdapterRequest)]
        L.ccsx_submit_screen.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(CExtras), C.POINTER(CFoldRequest), C.POINTER(CAdapterRequest),
                                         C.POINTER(C.c_int64)]
        L.ccsx_control_opts_default.restype = None
        L.ccsx_control_opts_default.argtypes = [C.POINTER(ControlOpts)]
        L.ccsx_consensus_control.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(CExtras), C.POINTER(CFoldRequest), C.POINTER(CAdapterRequest),
                                             C.POINTER(CControlRequest)]
        L.ccsx_submit_control.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(CExtras), C.POINTER(CFoldRequest), C.POINTER(CAdapterRequest),
                                          C.POINTER(CControlRequest), C.POINTER(C.c_int64)]
        L.ccsx_coverage_opts_default.restype = None
        L.ccsx_coverage_opts_default.argtypes = [C.POINTER(CoverageOpts)]
        L.ccsx_consensus_requests.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(CRequests)]
        L.ccsx_submit_requests.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(CRequests), C.POINTER(C.c_int64)]
        L.ccsx_handoff_opts_default.restype = None
        L.ccsx_handoff_opts_default.argtypes = [C.POINTER(HandoffOpts)]
        L.ccsx_consensus_handoff.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(CRequests), C.POINTER(CHandoffRequest)]
        L.ccsx_submit_handoff.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(CRequests), C.POINTER(CHandoffRequest), C.POINTER(C.c_int64)]
        L.ccsx_refine_tiles_init.restype = None
        L.ccsx_refine_tiles_init.argtypes = [C.POINTER(CRefineTiles)]
        L.ccsx_refine_perr.restype = C.c_uint64
        L.ccsx_refine_perr.argtypes = [C.c_int32]
        _refine = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(C.c_int32), C.POINTER(CRefineTiles), C.POINTER(CResults), C.POINTER(CRefineReport)]
        L.ccsx_refine_batch.argtypes = _refine
        L.ccsx_submit_refine.argtypes = _refine + [C.POINTER(C.c_int64)]
        L.ccsx_orient_opts_default.restype = None
        L.ccsx_orient_opts_default.argtypes = [C.POINTER(OrientOpts)]
        L.ccsx_orient_batch.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(OrientOpts), C.POINTER(COrientReport)]
        L.ccsx_set_orient_opts.argtypes = [C.c_void_p, C.POINTER(OrientOpts)]
        L.ccsx_stage_orient.argtypes = [C.c_void_p, C.POINTER(COrientReport)]
        _call = [C.POINTER(C.c_uint8), C.c_int64, C.POINTER(DeflateBlock), C.c_int32, C.POINTER(C.c_uint8), C.c_int64, C.POINTER(C.c_int32)]
        L.ccsx_inflater_create.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_void_p)]
        L.ccsx_inflater_destroy.argtypes = [C.c_void_p]
        L.ccsx_inflate_blocks.argtypes = [C.c_void_p] + _call
        L.ccsx_inflate_submit.argtypes = [C.c_void_p] + _call + [C.POINTER(C.c_int64)]
        L.ccsx_inflate_wait.argtypes = [C.c_void_p, C.c_int64]
        L.ccsx_inflate_blocks_host.argtypes = _call
        _dcall = [C.POINTER(C.c_uint8), C.c_int64, C.POINTER(DeflateSpan), C.c_int32, C.POINTER(C.c_uint8), C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_uint32),
                  C.POINTER(C.c_int32)]
        L.ccsx_deflate_bound.restype = C.c_int32
        L.ccsx_deflate_bound.argtypes = [C.c_int32]
        L.ccsx_deflater_create.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_void_p)]
        L.ccsx_deflater_destroy.argtypes = [C.c_void_p]
        L.ccsx_deflate_spans.argtypes = [C.c_void_p] + _dcall
        L.ccsx_deflate_submit.argtypes = [C.c_void_p] + _dcall + [C.POINTER(C.c_int64)]
        L.ccsx_deflate_wait.argtypes = [C.c_void_p, C.c_int64]
        L.ccsx_deflate_spans_host.argtypes = _dcall
        L.ccsx_deflate_crc.restype = C.c_uint32
        L.ccsx_deflate_crc.argtypes = [C.POINTER(C.c_uint8), C.c_int64]
        L.ccsx_deflate_code_lengths.argtypes = [C.POINTER(C.c_uint32), C.c_int32, C.c_int32, C.POINTER(C.c_uint8)]
        L.ccsx_deflate_fill_spans.restype = C.c_int32
        L.ccsx_deflate_fill_spans.argtypes = [C.c_int]
        _i64p = C.POINTER(C.c_int64)
        L.ccsx_train_batch.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CDrafts), C.POINTER(CTrainCounts)]
        L.ccsx_train_pair_host.argtypes = [C.POINTER(Model), C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                           C.POINTER(C.c_uint8), C.c_int32, C.c_float, _i64p, _i64p, _i64p, _i64p]
        L.ccsx_fit_opts_default.restype = None
        L.ccsx_fit_opts_default.argtypes = [C.POINTER(FitOpts)]
        L.ccsx_fitter_create.argtypes = [C.POINTER(Model), C.POINTER(FitOpts), C.POINTER(C.c_void_p)]
        L.ccsx_fitter_add.argtypes = [C.c_void_p, C.POINTER(CTrainCounts), C.POINTER(C.c_float)]
        L.ccsx_fitter_finish.argtypes = [C.c_void_p, C.POINTER(Model), C.POINTER(FitReport)]
        L.ccsx_fitter_destroy.argtypes = [C.c_void_p]
        L.ccsx_dup_opts_default.restype = None
        L.ccsx_dup_opts_default.argtypes = [C.POINTER(DupOpts)]
        L.ccsx_dup_hash.restype = C.c_uint32
        L.ccsx_dup_hash.argtypes = [C.c_uint32]
        _dsign = [C.POINTER(DupOpts), C.POINTER(C.c_uint8), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int32, C.c_void_p]
        _dclus = [C.POINTER(DupOpts), C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, C.POINTER(CDupReport)]
        L.ccsx_dup_sign_reads_host.argtypes = _dsign
        L.ccsx_dup_sign_reads.argtypes = [C.c_void_p] + _dsign
        L.ccsx_dup_cluster_host.argtypes = _dclus
        L.ccsx_dup_cluster.argtypes = [C.c_void_p] + _dclus
        L.ccsx_barcode_opts_default.restype = None
        L.ccsx_barcode_opts_default.argtypes = [C.POINTER(BarcodeOpts)]
        _bcreads = [C.POINTER(BarcodeSet), C.POINTER(BarcodeOpts), C.POINTER(C.c_uint8), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int32, C.POINTER(CBarcodeReport)]
        L.ccsx_barcode_reads_host.argtypes = _bcreads
        L.ccsx_barcode_reads.argtypes = [C.c_void_p] + _bcreads
        L.ccsx_consensus_barcodes.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(CRequests), C.POINTER(CBarcodeRequest)]
        L.ccsx_submit_barcodes.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(CRequests), C.POINTER(CBarcodeRequest), C.POINTER(C.c_int64)]
        L.ccsx_segment_opts_default.restype = None
        L.ccsx_segment_opts_default.argtypes = [C.POINTER(SegmentOpts)]
        _sgreads = [C.POINTER(SegmentSet), C.POINTER(SegmentOpts), C.POINTER(C.c_uint8), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int32, C.POINTER(CSegmentReport)]
        L.ccsx_segment_reads_host.argtypes = _sgreads
        L.ccsx_segment_reads.argtypes = [C.c_void_p] + _sgreads
        L.ccsx_consensus_segments.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(CRequests), C.POINTER(CSegmentRequest)]
        L.ccsx_submit_segments.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(CRequests), C.POINTER(CSegmentRequest), C.POINTER(C.c_int64)]
        L.ccsx_cell_design_default.restype = None
        L.ccsx_cell_design_default.argtypes = [C.POINTER(CellDesign)]
        L.ccsx_cell_slot.restype = C.c_uint32
        L.ccsx_cell_slot.argtypes = [C.c_uint32, C.c_uint32]
        L.ccsx_cell_whitelist_create.restype = C.c_void_p
        L.ccsx_cell_whitelist_create.argtypes = [C.POINTER(C.c_uint8), C.c_int32, C.c_int32]
        L.ccsx_cell_whitelist_destroy.restype = None
        L.ccsx_cell_whitelist_destroy.argtypes = [C.c_void_p]
        L.ccsx_cell_whitelist_info.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.POINTER(C.c_uint64))]
        _clreads = [C.POINTER(CdnaPrimers), C.POINTER(CdnaOpts), C.POINTER(CellDesign), C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                    C.c_int32, C.POINTER(CCellReport)]
        L.ccsx_cell_reads_host.argtypes = _clreads
        L.ccsx_cell_reads.argtypes = [C.c_void_p] + _clreads
        L.ccsx_cdna_opts_default.restype = None
        L.ccsx_cdna_opts_default.argtypes = [C.POINTER(CdnaOpts)]
        _cdreads = [C.POINTER(CdnaPrimers), C.POINTER(CdnaOpts), C.POINTER(C.c_uint8), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int32, C.POINTER(CCdnaReport)]
        L.ccsx_cdna_reads_host.argtypes = _cdreads
        L.ccsx_cdna_reads.argtypes = [C.c_void_p] + _cdreads
        L.ccsx_consensus_cdna.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(CRequests), C.POINTER(CCdnaRequest)]
        L.ccsx_submit_cdna.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(CRequests), C.POINTER(CCdnaRequest), C.POINTER(C.c_int64)]
        L.ccsx_represent_host.argtypes = [C.POINTER(CBatch), C.POINTER(Opts), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                                          C.POINTER(CRepresentRequest), C.POINTER(CResults)]
        L.ccsx_consensus_represent.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(CRequests), C.POINTER(CRepresentRequest)]
        L.ccsx_submit_represent.argtypes = [C.c_void_p, C.POINTER(CBatch), C.POINTER(CResults), C.POINTER(CRequests), C.POINTER(CRepresentRequest), C.POINTER(C.c_int64)]
        _lib = L
    return _lib


def _ptr(a: np.ndarray, ty):
    return a.ctypes.data_as(C.POINTER(ty))


class _Pinned:
    """Owner of one ccsx_alloc_pinned block."""

    def __init__(self, p):
        self.p = p

    def __del__(self):
        try:
            if self.p:
                lib().ccsx_free_pinned(self.p)
                self.p = None
        except Exception:
            pass


@dataclass
class Batch:
    """Input batch, SoA + CSR (include/ccsx.h ccsx_batch).  All arrays are C-contiguous numpy."""
    zmw_id: np.ndarray
    snr: np.ndarray
    read_off: np.ndarray
    base_off: np.ndarray
    bases: np.ndarray
    pw: np.ndarray
    ipd: np.ndarray
    flags: np.ndarray
    tpl_off: np.ndarray | None = None
    tpl: np.ndarray | None = None

    @property
    def n_zmw(self) -> int:
        return len(self.zmw_id)

    def c_struct(self) -> CBatch:
        b = CBatch()
        b.n_zmw = self.n_zmw
        b.n_reads = int(self.read_off[-1])
        b.n_bases = int(self.base_off[-1])
        b.zmw_id = _ptr(self.zmw_id, C.c_int32)
        b.snr = _ptr(self.snr, C.c_float)
        b.read_off = _ptr(self.read_off, C.c_int32)
        b.base_off = _ptr(self.base_off, C.c_int64)
        b.bases = _ptr(self.bases, C.c_uint8)
        b.pw = _ptr(self.pw, C.c_uint8)
        b.ipd = _ptr(self.ipd, C.c_uint8)
        b.flags = _ptr(self.flags, C.c_uint8)
        return b

    def read(self, r: int):
        a, b = int(self.base_off[r]), int(self.base_off[r + 1])
        return self.bases[a:b], self.pw[a:b]

    def algorithmic_bytes(self) -> int:
        """3*sum(len) + per ZMW (16 + 2*L_out + 32); L_out ~ template length."""
        n = self.n_zmw
        if self.tpl_off is not None:
            lout = int(self.tpl_off[-1])
        else:
            lout = int(self.base_off[-1]) // max(1, int(self.read_off[-1])) * n
        return 3 * int(self.base_off[-1]) + 48 * n + 2 * lout

    def pinned(self) -> "Batch":
        """Copy of this batch whose per-base arrays live in page-locked host memory (ccsx_alloc_pinned): uploads run at PCIe
        rate instead of through the runtime's pageable staging.  The buffers are released with the returned object."""
        L = lib()
        out = Batch(self.zmw_id, self.snr, self.read_off, self.base_off, None, None, None, self.flags, self.tpl_off, self.tpl)
        keep = []
        for name in ("bases", "pw", "ipd"):
            src = getattr(self, name)
            n = max(1, src.nbytes)
            p = L.ccsx_alloc_pinned(n)
            if not p:
                raise RuntimeError("ccsx_alloc_pinned failed: " + L.ccsx_last_error().decode())
            keep.append(_Pinned(p))
            arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n,))[: len(src)]
            arr[:] = src
            setattr(out, name, arr)
        out._pinned = keep
        return out

    def with_unknown_strands(self, guess=None) -> "Batch":
        """a copy whose every pass carries PASS_STRAND_UNKNOWN; guess (one value per pass, or None: the batch's own bits) replaces bit 0, now only a prior"""
        f = self.flags.copy()
        if guess is not None:
            f = (f & np.uint8(0xfe)) | (np.asarray(guess).astype(np.uint8) & np.uint8(1))
        out = replace(self, flags=np.ascontiguousarray(f | np.uint8(PASS_STRAND_UNKNOWN)))
        if hasattr(self, "_pinned"):
            out._pinned = self._pinned                   # (the copy shares the page-locked arrays)
        return out

    def slice(self, z0: int, z1: int) -> "Batch":
        r0, r1 = int(self.read_off[z0]), int(self.read_off[z1])
        b0, b1 = int(self.base_off[r0]), int(self.base_off[r1])
        kw = {}
        if self.tpl_off is not None:
            t0, t1 = int(self.tpl_off[z0]), int(self.tpl_off[z1])
            kw = dict(tpl_off=(self.tpl_off[z0:z1 + 1] - t0).copy(), tpl=self.tpl[t0:t1].copy())
        return Batch(self.zmw_id[z0:z1].copy(), self.snr[z0:z1].copy(), (self.read_off[z0:z1 + 1] - r0).copy(),
                     (self.base_off[r0:r1 + 1] - b0).copy(), self.bases[b0:b1].copy(), self.pw[b0:b1].copy(),
                     self.ipd[b0:b1].copy(), self.flags[r0:r1].copy(), **kw)


def concat(parts) -> "Batch":
    """the ZMWs of several batches as one batch, in order (ZMW ids are renumbered 0..n-1)"""
    read_off, base_off, tpl_off = [np.zeros(1, np.int32)], [np.zeros(1, np.int64)], [np.zeros(1, np.int64)]
    for b in parts:
        read_off.append(b.read_off[1:] + read_off[-1][-1]); base_off.append(b.base_off[1:] + base_off[-1][-1])
        tpl_off.append(b.tpl_off[1:] + tpl_off[-1][-1])
    cat = lambda k: np.ascontiguousarray(np.concatenate([getattr(b, k) for b in parts]))
    n = sum(b.n_zmw for b in parts)
    return Batch(np.arange(n, dtype=np.int32), cat("snr"), np.concatenate(read_off).astype(np.int32), np.concatenate(base_off).astype(np.int64),
                 cat("bases"), cat("pw"), cat("ipd"), cat("flags"), np.concatenate(tpl_off).astype(np.int64), cat("tpl"))


def synth(n_zmw: int, passes, length, seed: int = 1, first_zmw_id: int = 0) -> Batch:
    """Deterministic synthetic subreads (ccsx_synth_generate).  passes/length: int or (lo, hi)."""
    plo, phi = (passes, passes) if isinstance(passes, int) else passes
    llo, lhi = (length, length) if isinstance(length, int) else length
    L = lib()
    p = C.POINTER(CSynth)()
    if L.ccsx_synth_generate(n_zmw, first_zmw_id, plo, phi, llo, lhi, seed, C.byref(p)) != 0:
        raise RuntimeError(L.ccsx_last_error().decode())
    s = p.contents
    b = s.batch
    R, NB = b.n_reads, b.n_bases

    def cp(ptr, n, dt):
        return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dt)

    out = Batch(cp(b.zmw_id, n_zmw, np.int32), cp(b.snr, 4 * n_zmw, np.float32).reshape(n_zmw, 4),
                cp(b.read_off, n_zmw + 1, np.int32), cp(b.base_off, R + 1, np.int64), cp(b.bases, NB, np.uint8),
                cp(b.pw, NB, np.uint8), cp(b.ipd, NB, np.uint8), cp(b.flags, R, np.uint8),
                tpl_off=cp(s.tpl_off, n_zmw + 1, np.int64))
    out.tpl = cp(s.tpl, int(out.tpl_off[-1]), np.uint8)
    L.ccsx_synth_free(p)
    return out


def default_model() -> Model:
    m = Model()
    lib().ccsx_model_default(C.byref(m))
    return m


def set_model_name(m: Model, name: str) -> Model:
    """name of a parameter set, zero padded (the blob is compared / hashed as bytes; ctypes assignment stops at the first NUL)"""
    raw = name.encode()[:31].ljust(32, b"\0")
    C.memmove(C.addressof(m), raw, 32)
    return m


def model_to_json(m: Model, chemistry=None) -> str:
    """json text of a parameter set (ccsx_model_to_json); chemistry = (binding kit, sequencing kit, basecaller version) or None"""
    L = lib()
    tri = [c.encode() for c in chemistry] if chemistry else [None, None, None]
    n = L.ccsx_model_to_json(C.byref(m), *tri, None, 0)
    buf = C.create_string_buffer(n + 1)
    L.ccsx_model_to_json(C.byref(m), *tri, buf, n + 1)
    return buf.value.decode()


def model_from_json(text: str) -> Model:
    m = Model()
    if lib().ccsx_model_from_json(text.encode(), C.byref(m)) != 0:
        raise RuntimeError(lib().ccsx_last_error().decode())
    return m


def model_load(path: str) -> Model:
    m = Model()
    if lib().ccsx_model_load(path.encode(), C.byref(m)) != 0:
        raise RuntimeError(lib().ccsx_last_error().decode())
    return m


def model_for_chemistry(binding_kit: str, sequencing_kit: str, basecaller_version: str) -> Model:
    m = Model()
    if lib().ccsx_model_for_chemistry(binding_kit.encode(), sequencing_kit.encode(), basecaller_version.encode(), C.byref(m)) != 0:
        raise RuntimeError(lib().ccsx_last_error().decode())
    return m


def default_opts() -> Opts:
    o = Opts()
    lib().ccsx_opts_default(C.byref(o))
    return o


@dataclass
class Results:
    seq_off: np.ndarray
    status: np.ndarray
    seq_len: np.ndarray
    seq: np.ndarray
    qual: np.ndarray
    raw_qv: np.ndarray
    rq: np.ndarray
    np_: np.ndarray
    ec: np.ndarray
    iters: np.ndarray
    n_windows: np.ndarray
    fn: np.ndarray = None
    rn: np.ndarray = None
    kin: np.ndarray | None = None        # [4, capacity] planes fi, fp, ri, rp (CodecV1 codes); None without kinetics

    @staticmethod
    def allocate(batch: Batch, kinetics: bool = False, pinned: bool = False, raw: bool = True) -> "Results":
        """pinned=True puts every array in page-locked memory (ccsx_alloc_pinned): asynchronous downloads (Handle.submit)
        then run by DMA at PCIe rate."""
        n = batch.n_zmw
        cb = batch.c_struct()
        off = np.zeros(n + 1, np.int64)
        cap = lib().ccsx_result_layout(C.byref(cb), _ptr(off, C.c_int64))
        keep = []

        def z(shape, dt):
            if not pinned:
                return np.zeros(shape, dt)
            nb = max(1, int(np.prod(shape)) * np.dtype(dt).itemsize)
            p = lib().ccsx_alloc_pinned(nb)
            if not p:
                raise RuntimeError("ccsx_alloc_pinned failed: " + lib().ccsx_last_error().decode())
            keep.append(_Pinned(p))
            a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(nb,))[: int(np.prod(shape)) * np.dtype(dt).itemsize]
            a = a.view(dt).reshape(shape)
            a[...] = 0
            return a
        r = Results(off, z(n, np.int32), z(n, np.int32), z(cap, np.uint8), z(cap, np.uint8),
                    z(cap, np.float32) if raw else None, z(n, np.float32), z(n, np.int32), z(n, np.float32),
                    z(n, np.int32), z(n, np.int32), z(n, np.int32), z(n, np.int32),
                    z((4, cap), np.uint8) if kinetics else None)
        r._pinned = keep
        return r

    def c_struct(self) -> CResults:
        r = CResults()
        r.n_zmw = len(self.status)
        r.seq_capacity = len(self.seq)
        r.seq_off = _ptr(self.seq_off, C.c_int64)
        r.status = _ptr(self.status, C.c_int32)
        r.seq_len = _ptr(self.seq_len, C.c_int32)
        r.seq = _ptr(self.seq, C.c_uint8)
        r.qual = _ptr(self.qual, C.c_uint8)
        r.raw_qv = _ptr(self.raw_qv, C.c_float) if self.raw_qv is not None else None   # optional output: NULL = not downloaded
        r.rq = _ptr(self.rq, C.c_float)
        r.np = _ptr(self.np_, C.c_int32)
        r.ec = _ptr(self.ec, C.c_float)
        r.iters = _ptr(self.iters, C.c_int32)
        r.n_windows = _ptr(self.n_windows, C.c_int32)
        r.fn = _ptr(self.fn, C.c_int32)
        r.rn = _ptr(self.rn, C.c_int32)
        if self.kin is not None:
            r.fi, r.fp, r.ri, r.rp = (_ptr(self.kin[k], C.c_uint8) for k in range(4))
        return r

    def sequence(self, z: int) -> np.ndarray:
        o = int(self.seq_off[z])
        return self.seq[o:o + int(self.seq_len[z])]

    def quals(self, z: int) -> np.ndarray:
        o = int(self.seq_off[z])
        return self.qual[o:o + int(self.seq_len[z])]

    def raw(self, z: int) -> np.ndarray:
        o = int(self.seq_off[z])
        return self.raw_qv[o:o + int(self.seq_len[z])]

    def kinetics(self, z: int) -> np.ndarray:
        """[4, seq_len] CodecV1 codes (fi, fp, ri, rp) of ZMW z, orientation of SEQ."""
        o = int(self.seq_off[z])
        return self.kin[:, o:o + int(self.seq_len[z])]


@dataclass
class Drafts:
    """ccsx_drafts: what the draft seam hands to the polish seam (include/ccsx.h)."""
    seq_off: np.ndarray
    win_off: np.ndarray
    status: np.ndarray
    len: np.ndarray
    seq: np.ndarray
    backbone: np.ndarray
    n_windows: np.ndarray
    win_bounds: np.ndarray

    @staticmethod
    def allocate(batch: Batch, pinned: bool | None = None) -> "Drafts":
        """pinned (default wherever there is a device): the arrays the ticketed seams copy asynchronously live in page-locked memory, as include/ccsx.h asks
        (with pageable arrays the copies block the submitting thread until the stage has finished)"""
        if pinned is None:
            pinned = lib().ccsx_device_count() > 0
        n = batch.n_zmw
        cb = batch.c_struct()
        so, wo = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
        sc, wc = C.c_int64(), C.c_int64()
        lib().ccsx_draft_layout(C.byref(cb), _ptr(so, C.c_int64), _ptr(wo, C.c_int64), C.byref(sc), C.byref(wc))
        keep = []

        def z(count, dt):
            if not pinned:
                return np.zeros(count, dt)
            nb = max(1, int(count) * np.dtype(dt).itemsize)
            p = lib().ccsx_alloc_pinned(nb)
            if not p:
                raise RuntimeError("ccsx_alloc_pinned failed: " + lib().ccsx_last_error().decode())
            keep.append(_Pinned(p))
            a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(nb,))[: int(count) * np.dtype(dt).itemsize].view(dt)
            a[...] = 0
            return a
        d = Drafts(so, wo, z(n, np.int32), z(n, np.int32), z(sc.value, np.uint8), z(n, np.int32), z(n, np.int32), z(wc.value, np.int32))
        d._pinned = keep
        return d

    def c_struct(self) -> CDrafts:
        d = CDrafts()
        d.n_zmw = len(self.len); d.seq_capacity = len(self.seq); d.win_capacity = len(self.win_bounds)
        d.seq_off = _ptr(self.seq_off, C.c_int64); d.win_off = _ptr(self.win_off, C.c_int64)
        d.status = _ptr(self.status, C.c_int32); d.len = _ptr(self.len, C.c_int32); d.seq = _ptr(self.seq, C.c_uint8)
        d.backbone = _ptr(self.backbone, C.c_int32); d.n_windows = _ptr(self.n_windows, C.c_int32); d.win_bounds = _ptr(self.win_bounds, C.c_int32)
        return d

    def draft(self, z: int) -> np.ndarray:
        o = int(self.seq_off[z])
        return self.seq[o:o + int(self.len[z])]

    def set_draft(self, z: int, bases: np.ndarray, backbone: int = 0):
        o = int(self.seq_off[z])
        assert len(bases) <= int(self.seq_off[z + 1]) - o
        self.seq[o:o + len(bases)] = bases
        self.len[z] = len(bases); self.backbone[z] = backbone

    def windows(self, z: int) -> np.ndarray:
        o = int(self.win_off[z])
        return self.win_bounds[o:o + int(self.n_windows[z]) + 1]


def _extras(cp: "CPileup | None", tandem: "np.ndarray | None", min_len: int) -> CExtras:
    ex = CExtras()
    ex.pile = C.pointer(cp) if cp is not None else None
    ex.tandem_len = _ptr(tandem, C.c_int32) if tandem is not None else None
    ex.min_tandem_repeat_length = int(min_len)
    ex.reserved = 0
    return ex


def _requests(pileup: "Pileup | None" = None, tandem: "np.ndarray | None" = None, min_tandem_repeat_length: int = 0,
              hd: "HdReport | None" = None, hd_opts: "HdOpts | None" = None, hd_split: bool = False,
              fold: "FoldReport | None" = None, fold_opts: "FoldOpts | None" = None,
              adapters: "AdapterReport | None" = None, adapter_set: "AdapterSet | None" = None, adapter_opts: "AdapterOpts | None" = None,
              control: "ControlReport | None" = None, control_seq: "ControlSeq | None" = None, control_opts: "ControlOpts | None" = None,
              coverage: "CoverageReport | None" = None, coverage_opts: "CoverageOpts | None" = None, coverage_gate: int = 0, via_requests: bool = False,
              hd_requests: bool = False):
    """The ctypes side of what one fused run is asked for beside the consensus: (CExtras, CHdRequest, CFoldRequest, CAdapterRequest, CControlRequest, keep), each
    request None where its report (for the extras: all of pileup, tandem and the threshold) is.  keep owns every array and struct the requests point to: it
    must outlive the call, or the ticket.  With a coverage report, or via_requests, or a heteroduplex request beside a screen, keep ends with the CRequests
    that carries every member but the heteroduplex request (ccsx_*_requests).  A heteroduplex request beside a CRequests is for ccsx_*_hd_requests, which takes
    it as a further argument: the caller says so with hd_requests=True (Handle._fused then picks that entry point); without it the combination is refused"""
    keep = [pileup, tandem, hd, fold, adapters, control, coverage]

    def own(x):
        keep.append(x)
        return x
    ex = hq = fq = aq = cq = None
    if pileup is not None or tandem is not None or min_tandem_repeat_length:
        ex = own(_extras(own(pileup.c_struct()) if pileup is not None else None, tandem, min_tandem_repeat_length))
    if hd is not None:
        o = own(hd_opts if hd_opts is not None else hd_opts_default())
        hq = own(CHdRequest(C.pointer(o), C.pointer(own(hd.c_struct())), int(bool(hd_split)), 0))
    if fold is not None:
        fq = own(_fold_request(fold_opts, own(fold.c_struct())))[0]
    if adapters is not None:
        aq = own(_adapter_request(adapter_set, adapter_opts, own(adapters.c_struct())))[0]
    if control is not None:
        cq = own(_control_request(control_seq, control_opts, own(control.c_struct())))[0]
    if coverage is not None or via_requests or (hq is not None and (fq is not None or aq is not None or cq is not None)):
        if hq is not None and not hd_requests:
            raise ValueError("the heteroduplex request goes beside ccsx_requests, through ccsx_*_hd_requests (hd_requests=True), not inside it")
        vq = own(_coverage_request(coverage_opts, coverage_gate, own(coverage.c_struct())))[0] if coverage is not None else None

        def p(x):
            return C.pointer(x) if x is not None else None
        keep.append(CRequests(p(ex), p(fq), p(aq), p(cq), p(vq), (C.c_void_p * 3)()))
    return ex, hq, fq, aq, cq, keep



def _reads_request(key: str, set_kw: str):
    """how Handle._fused builds the request of an analysis on final reads from (report, set, opts); set_kw: Handle.submit's keyword for the set"""
    def build(what):
        rep, pset, opts = what
        if pset is None:
            raise ValueError(f"{key}: a {set_kw} is needed")
        return _pattern_request(type(rep), pset, opts, rep.c_struct()) + (rep,)
    return build


# The requests of which a fused run takes one at most, and none beside the heteroduplex request, as Handle._fused walks them: its keyword there (ccsx_*_<keyword>
# is the entry point), how the refusal of a combination begins, and how its value becomes the C request (first element) and what must outlive the call
_EXCLUSIVE = (("handoff", "the heteroduplex request and the hand-off are not combined", _handoff_request),
              ("barcodes", "the barcode request is not combined", _reads_request("barcodes", "barcode_set")),
              ("represent", "the represent request is not combined", lambda what: _represent_request(*what)),
              ("segments", "the segment request is not combined", _reads_request("segments", "segment_set")),
              ("cdna", "the cdna request is not combined", _reads_request("cdna", "cdna_primers")))


def _exclusive(other: bool, handoff=None, barcodes=None, represent=None, segments=None, cdna=None):
    """the one request of _EXCLUSIVE among the arguments, as (row, value), or None.  ValueError for two of them, and for one when `other`: the run carries
    the heteroduplex request (or goes through an entry point that does not take a ccsx_requests)"""
    asked = [(row, what) for row, what in zip(_EXCLUSIVE, (handoff, barcodes, represent, segments, cdna)) if what is not None]
    if asked and (len(asked) > 1 or other):
        raise ValueError(asked[-1][0][1] + ": a run takes one of the hand-off, the barcode, the represent, the segment and the cdna request, beside the members of "
                         "ccsx_requests and without the heteroduplex request")
    return asked[-1] if asked else None


class Handle:
    """One consensus engine bound to one GPU (ccsx_create).  Not thread-safe: one per worker per GPU."""

    def __init__(self, device: int = 0, model: Model | None = None, opts: Opts | None = None):
        self._L = lib()
        self.device = int(device)
        self.model = model or default_model()
        self.opts = opts or default_opts()
        self._h = C.c_void_p()
        rc = self._L.ccsx_create(device, C.byref(self.model), C.byref(self.opts), C.byref(self._h))
        if rc != 0:
            raise RuntimeError("ccsx_create failed: " + self._L.ccsx_last_error().decode())
        self._keep = None
        self._sync_reads = 0                             # passes of the last batch staged on slot 0 (stage_orient)

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed: " + self._L.ccsx_last_error().decode())

    def _fused(self, form: str, batch: Batch, res: "Results", requests, *ticket, handoff: "Handoff | None" = None, barcodes=None, represent=None, segments=None, cdna=None):
        """One fused run (form 'consensus', or 'submit' with the ticket to fill) through the most general entry point that takes what _requests made:
        ccsx_*_hd with a heteroduplex request and nothing but extras, ccsx_*_requests when _requests made a CRequests (a coverage request, or
        via_requests; ccsx_*_hd_requests when a heteroduplex request goes with it), else ccsx_*_control (NULL: not asked for).  handoff: through ccsx_*_handoff, with the CRequests _requests made (via_requests); its
        structs join the requests' keep list.  barcodes: (report, set, opts), through ccsx_*_barcodes in the same way (not together with a hand-off).
        represent: (report, subread_fallback, kinetics), through ccsx_*_represent in the same way (not together with a hand-off or barcodes).
        segments: (report, set, opts), through ccsx_*_segments in the same way (not together with a hand-off, barcodes or represent).
        cdna: (report, primers, opts), through ccsx_*_cdna in the same way (not together with any of the four).  Returns the C structs"""
        ex, hq, fq, aq, cq, _keep = requests
        name, args = (f"ccsx_{form}_hd", (ex, hq)) if hq is not None else (f"ccsx_{form}_control", (ex, fq, aq, cq))
        if _keep and isinstance(_keep[-1], CRequests):
            name, args = (f"ccsx_{form}_hd_requests", (_keep[-1], hq)) if hq is not None else (f"ccsx_{form}_requests", (_keep[-1],))
        one = _exclusive(name != f"ccsx_{form}_requests", handoff, barcodes, represent, segments, cdna)
        if one is not None:
            (key, _, build), what = one
            req = build(what)
            name, args = f"ccsx_{form}_{key}", (_keep[-1], req[0])
            _keep.append(req)
        cb, cr = batch.c_struct(), res.c_struct()
        self._check(getattr(self._L, name)(self._h, cb, cr, *args, *ticket), name)
        if form == "consensus":
            self._sync_reads = int(batch.read_off[-1])
        return cb, cr

    def consensus(self, batch: Batch) -> Results:
        res = Results.allocate(batch, kinetics=bool(self.opts.hifi_kinetics))
        cb, cr = batch.c_struct(), res.c_struct()
        self._check(self._L.ccsx_consensus_batch(self._h, C.byref(cb), C.byref(cr)), "ccsx_consensus_batch")
        self._sync_reads = int(batch.read_off[-1])
        return res

    # ---- the two seams (docs/img/ccs-impl.png): draft stage alone, polish stage on caller-supplied drafts
    def draft(self, batch: Batch) -> "Drafts":
        d = Drafts.allocate(batch)
        cb, cd = batch.c_struct(), d.c_struct()
        self._check(self._L.ccsx_draft_batch(self._h, C.byref(cb), C.byref(cd)), "ccsx_draft_batch")
        return d

    def polish(self, batch: Batch, drafts: "Drafts", flags: int = 0) -> Results:
        res = Results.allocate(batch, kinetics=bool(self.opts.hifi_kinetics))
        cb, cd, cr = batch.c_struct(), drafts.c_struct(), res.c_struct()
        self._check(self._L.ccsx_polish_batch(self._h, C.byref(cb), C.byref(cd), C.byref(cr), flags), "ccsx_polish_batch")
        return res

    # ---- the third seam: the heteroduplex finder on caller-supplied drafts (no polish runs)
    def hd(self, batch: Batch, drafts: "Drafts", opts: HdOpts | None = None) -> HdReport:
        rep = HdReport.allocate(batch.n_zmw)
        cb, cd, cr = batch.c_struct(), drafts.c_struct(), rep.c_struct()
        o = opts if opts is not None else hd_opts_default()
        self._check(self._L.ccsx_hd_batch(self._h, C.byref(cb), C.byref(cd), C.byref(o), C.byref(cr)), "ccsx_hd_batch")
        self._sync_reads = int(batch.read_off[-1])
        return rep

    # ---- the fourth seam: the training counts on caller-supplied drafts (no polish runs; DESIGN.md §2 "Model training")
    def train_counts(self, batch: Batch, drafts: "Drafts") -> TrainCounts:
        tc = TrainCounts.allocate(batch)
        cb, cd, cc = batch.c_struct(), drafts.c_struct(), tc.c_struct()
        self._check(self._L.ccsx_train_batch(self._h, C.byref(cb), C.byref(cd), C.byref(cc)), "ccsx_train_batch")
        self._sync_reads = int(batch.read_off[-1])
        return tc

    # ---- pass orientation (DESIGN.md §2 "Pass orientation"): the seam, the options of every other path, the last synchronous run's report
    def orient(self, batch: Batch, opts: "OrientOpts | None" = None) -> OrientReport:
        rep = OrientReport.allocate(int(batch.read_off[-1]))
        cb, cr = batch.c_struct(), rep.c_struct()
        self._check(self._L.ccsx_orient_batch(self._h, C.byref(cb), C.byref(opts) if opts is not None else None, C.byref(cr)), "ccsx_orient_batch")
        self._sync_reads = int(batch.read_off[-1])
        return rep

    def set_orient_opts(self, opts: "OrientOpts | None" = None):
        self._check(self._L.ccsx_set_orient_opts(self._h, C.byref(opts) if opts is not None else None), "ccsx_set_orient_opts")

    def stage_orient(self, n_reads: "int | None" = None) -> OrientReport:
        """the report of the last synchronous run on slot 0 (n_reads: its passes; None = those of the last batch this object ran synchronously)"""
        rep = OrientReport.allocate(self._sync_reads if n_reads is None else n_reads)
        cr = rep.c_struct()
        self._check(self._L.ccsx_stage_orient(self._h, C.byref(cr)), "ccsx_stage_orient")
        return rep

    # ---- the pileup summary (sa sm sx): the fused path plus per-base planes from the kinetics alignment
    def consensus_pileup(self, batch: Batch) -> tuple["Results", "Pileup"]:
        res = Results.allocate(batch, kinetics=bool(self.opts.hifi_kinetics))
        pile = Pileup.allocate(res)
        self._fused("consensus", batch, res, _requests(pile))
        return res, pile

    def _outputs(self, batch: Batch, tandem: bool, pileup: bool):
        """what a synchronous fused run fills: (results, tandem_len or None, pileup or None)"""
        res = Results.allocate(batch, kinetics=bool(self.opts.hifi_kinetics))
        return res, tandem_buffer(batch.n_zmw) if tandem else None, Pileup.allocate(res) if pileup else None

    # ---- optional outputs through ccsx_extras: tandem-repeat detection (DESIGN.md §2 "Tandem repeats") and / or the pileup summary
    def consensus_extras(self, batch: Batch, tandem: bool = True, min_tandem_repeat_length: int = 0,
                         pileup: bool = False) -> tuple["Results", "np.ndarray | None", "Pileup | None"]:
        """ccsx_consensus_extras: (results, tandem_len [n_zmw] int32 or None, pileup or None).  min_tandem_repeat_length > 0: ZMWs whose deciding
        draft has a masked run at least that long run with the heuristics off (as opts.disable_heuristics), the others as usual"""
        res, tl, pile = self._outputs(batch, tandem, pileup)
        self._fused("consensus", batch, res, _requests(pile, tl, min_tandem_repeat_length))
        return res, tl, pile

    # ---- the heteroduplex finder in the fused path (ccsx_consensus_hd): the consensus and the finder's report of one run
    def consensus_hd(self, batch: Batch, opts: HdOpts | None = None, split: bool = False, tandem: bool = False, min_tandem_repeat_length: int = 0,
                     pileup: bool = False) -> tuple["Results", HdReport, "np.ndarray | None", "Pileup | None"]:
        """(results, report, tandem_len or None, pileup or None).  split=True: a HETERODUPLEX ZMW is not polished (status HETERODUPLEX, no consensus);
        split=False: detection only, the results are those of consensus_extras"""
        res, tl, pile = self._outputs(batch, tandem, pileup)
        rep = HdReport.allocate(batch.n_zmw)
        self._fused("consensus", batch, res, _requests(pile, tl, min_tandem_repeat_length, hd=rep, hd_opts=opts, hd_split=split))
        return res, rep, tl, pile

    # ---- the finder beside the other requests (ccsx_consensus_hd_requests): one run with the finder and any of the screens
    def consensus_hd_requests(self, batch: Batch, opts: HdOpts | None = None, split: bool = False, coverage: "bool | CoverageOpts" = False, gate: int = 0,
                              control: "ControlSeq | None" = None, control_opts: "ControlOpts | None" = None, fold: "bool | FoldOpts" = False,
                              adapters: "AdapterSet | None" = None, adapter_opts: "AdapterOpts | None" = None, tandem: bool = False,
                              min_tandem_repeat_length: int = 0, pileup: bool = False, via_requests: bool = True):
        """(results, hd report, coverage report or None, control report or None, fold report or None, adapter report or None, tandem_len or None, pileup or
        None).  opts / split as consensus_hd; coverage: True or a CoverageOpts asks for the coverage screen, gate its gate; the other arguments as
        consensus_coverage.  The coverage gate gives its statuses before the finder's split does (include/ccsx.h).  via_requests=False: through
        ccsx_consensus_hd when nothing but extras goes with the finder"""
        res, tl, pile = self._outputs(batch, tandem, pileup)
        rep = HdReport.allocate(batch.n_zmw)
        vrep = CoverageReport.allocate(batch.n_zmw) if coverage else None
        crep = ControlReport.allocate(batch.n_zmw) if control is not None else None
        frep = FoldReport.allocate(batch.n_zmw) if fold else None
        arep = AdapterReport.allocate(batch.n_zmw) if adapters is not None else None
        self._fused("consensus", batch, res, _requests(pile, tl, min_tandem_repeat_length, hd=rep, hd_opts=opts, hd_split=split,
                                                       fold=frep, fold_opts=fold if isinstance(fold, FoldOpts) else None,
                                                       adapters=arep, adapter_set=adapters, adapter_opts=adapter_opts,
                                                       control=crep, control_seq=control, control_opts=control_opts,
                                                       coverage=vrep, coverage_opts=coverage if isinstance(coverage, CoverageOpts) else None,
                                                       coverage_gate=gate, via_requests=via_requests, hd_requests=True))
        return res, rep, vrep, crep, frep, arep, tl, pile

    # ---- adapter palindromes in the fused path (ccsx_consensus_fold): the consensus and the detector's report of one run (detection only)
    def consensus_fold(self, batch: Batch, opts: FoldOpts | None = None) -> tuple["Results", FoldReport]:
        res = Results.allocate(batch, kinetics=bool(self.opts.hifi_kinetics))
        rep = FoldReport.allocate(batch.n_zmw)
        self._fused("consensus", batch, res, _requests(fold=rep, fold_opts=opts))
        return res, rep

    # ---- both draft detectors in one run (ccsx_consensus_screen): adapter palindromes and / or the adapter screen, with the optional outputs of ccsx_extras
    def consensus_screen(self, batch: Batch, fold: "bool | FoldOpts" = False, adapters: "AdapterSet | None" = None, opts: "AdapterOpts | None" = None,
                         tandem: bool = False, min_tandem_repeat_length: int = 0, pileup: bool = False):
        """(results, fold report or None, adapter report or None, tandem_len or None, pileup or None).  fold: True or a FoldOpts asks for the palindrome
        report; adapters: an AdapterSet asks for the adapter screen (AdapterSet.default() = the SMRTbell hairpin), opts its AdapterOpts.  Detection only"""
        res, tl, pile = self._outputs(batch, tandem, pileup)
        frep = FoldReport.allocate(batch.n_zmw) if fold else None
        arep = AdapterReport.allocate(batch.n_zmw) if adapters is not None else None
        self._fused("consensus", batch, res, _requests(pile, tl, min_tandem_repeat_length, fold=frep, fold_opts=fold if isinstance(fold, FoldOpts) else None,
                                                       adapters=arep, adapter_set=adapters, adapter_opts=opts))
        return res, frep, arep, tl, pile

    # ---- the control screen (ccsx_consensus_control), alone or with the other draft detectors and the optional outputs of ccsx_extras
    def consensus_control(self, batch: Batch, control: ControlSeq, opts: "ControlOpts | None" = None, fold: "bool | FoldOpts" = False,
                          adapters: "AdapterSet | None" = None, adapter_opts: "AdapterOpts | None" = None, tandem: bool = False,
                          min_tandem_repeat_length: int = 0, pileup: bool = False):
        """(results, control report, fold report or None, adapter report or None, tandem_len or None, pileup or None).  control: the spike-in control
        (ControlSeq.from_string / from_codes), opts its ControlOpts; the other arguments as consensus_screen.  Detection only"""
        res, tl, pile = self._outputs(batch, tandem, pileup)
        crep = ControlReport.allocate(batch.n_zmw)
        frep = FoldReport.allocate(batch.n_zmw) if fold else None
        arep = AdapterReport.allocate(batch.n_zmw) if adapters is not None else None
        self._fused("consensus", batch, res, _requests(pile, tl, min_tandem_repeat_length, fold=frep, fold_opts=fold if isinstance(fold, FoldOpts) else None,
                                                       adapters=arep, adapter_set=adapters, adapter_opts=adapter_opts,
                                                       control=crep, control_seq=control, control_opts=opts))
        return res, crep, frep, arep, tl, pile

    # ---- the coverage screen (ccsx_consensus_requests), alone or with the draft detectors and the optional outputs of ccsx_extras
    def consensus_coverage(self, batch: Batch, opts: "CoverageOpts | None" = None, gate: int = 0, control: "ControlSeq | None" = None,
                           control_opts: "ControlOpts | None" = None, fold: "bool | FoldOpts" = False, adapters: "AdapterSet | None" = None,
                           adapter_opts: "AdapterOpts | None" = None, tandem: bool = False, min_tandem_repeat_length: int = 0, pileup: bool = False):
        """(results, coverage report, control report or None, fold report or None, adapter report or None, tandem_len or None, pileup or None).  opts: the
        CoverageOpts (None: the defaults); gate: bit v set gives a ZMW with verdict v = 2 .. 5 the status 9 + v and no consensus (COVERAGE_GATE_ALL: all four),
        0: detection only.  The other arguments as consensus_control (control: a ControlSeq asks for the control screen)"""
        res, tl, pile = self._outputs(batch, tandem, pileup)
        vrep = CoverageReport.allocate(batch.n_zmw)
        crep = ControlReport.allocate(batch.n_zmw) if control is not None else None
        frep = FoldReport.allocate(batch.n_zmw) if fold else None
        arep = AdapterReport.allocate(batch.n_zmw) if adapters is not None else None
        self._fused("consensus", batch, res, _requests(pile, tl, min_tandem_repeat_length, fold=frep, fold_opts=fold if isinstance(fold, FoldOpts) else None,
                                                       adapters=arep, adapter_set=adapters, adapter_opts=adapter_opts,
                                                       control=crep, control_seq=control, control_opts=control_opts,
                                                       coverage=vrep, coverage_opts=opts, coverage_gate=gate))
        return res, vrep, crep, frep, arep, tl, pile

    # ---- the polisher hand-off (ccsx_consensus_handoff): the low-quality tiles of the consensus as pass-by-column arrays, alone or with the requests above
    def consensus_handoff(self, batch: Batch, opts: "HandoffOpts | None" = None, max_tiles: "int | None" = None, device: bool = False,
                          handoff: "Handoff | None" = None, res: "Results | None" = None, **requests) -> tuple["Results", "Handoff"]:
        """(results, hand-off).  opts: the HandoffOpts (None: the defaults); max_tiles: the arrays' capacity (None: every tile the batch can have);
        device=True: the arrays are torch tensors on this handle's GPU.  handoff: a Handoff of the caller's instead; res: the caller's Results.  requests:
        Handle.submit's keyword arguments for the other requests of the same run (pileup=, tandem=, fold=, adapters=, control=, coverage= ... with their
        reports; not hd=)"""
        if res is None:
            res = Results.allocate(batch, kinetics=bool(self.opts.hifi_kinetics))
        ho = handoff if handoff is not None else Handoff.allocate(batch, max_tiles, opts, device=self.device if device else False)
        self._fused("consensus", batch, res, _requests(via_requests=True, **requests), handoff=ho)
        return res, ho

    # ---- the analyses on final reads: one fused run with the request `key` of _EXCLUSIVE, and the kernel alone on the caller's reads
    def _consensus_reads(self, key: str, rep_cls, batch: Batch, pset, opts, res, requests):
        if res is None:
            res = Results.allocate(batch, kinetics=bool(self.opts.hifi_kinetics))
        rep = rep_cls.allocate(batch.n_zmw)
        self._fused("consensus", batch, res, _requests(via_requests=True, **requests), **{key: (rep, pset, opts)})
        return res, rep

    def _reads(self, rep_cls, pset, reads, opts, report):
        args, rep, _keep = _reads_args(rep_cls, pset, opts, reads, report)
        self._check(getattr(self._L, rep_cls.READS)(self._h, *args), rep_cls.READS)
        return rep

    # ---- barcode calls (ccsx_consensus_barcodes / ccsx_barcode_reads): the barcodes at both ends of the final reads
    def consensus_barcodes(self, batch: Batch, bset: BarcodeSet, opts: "BarcodeOpts | None" = None, res: "Results | None" = None,
                           **requests) -> tuple["Results", BarcodeReport]:
        """(results, barcode report).  bset: the BarcodeSet; opts: the BarcodeOpts (None: the defaults); res: the caller's Results.  requests: Handle.submit's
        keyword arguments for the other requests of the same run (pileup=, tandem=, fold=, adapters=, control=, coverage= ... with their reports; not hd=,
        not handoff=)"""
        return self._consensus_reads("barcodes", BarcodeReport, batch, bset, opts, res, requests)

    # ---- segmentation (ccsx_consensus_segments / ccsx_segment_reads): the segments of concatenated-array reads
    def consensus_segments(self, batch: Batch, sset: SegmentSet, opts: "SegmentOpts | None" = None, res: "Results | None" = None,
                           **requests) -> tuple["Results", SegmentReport]:
        """(results, segment report).  sset: the SegmentSet; opts: the SegmentOpts (None: the defaults); res: the caller's Results.  requests: Handle.submit's
        keyword arguments for the other requests of the same run (pileup=, tandem=, fold=, adapters=, control=, coverage= ... with their reports; not hd=,
        handoff=, barcodes=, represent=)"""
        return self._consensus_reads("segments", SegmentReport, batch, sset, opts, res, requests)

    def segment_reads(self, sset: SegmentSet, reads, opts: "SegmentOpts | None" = None, report: "SegmentReport | None" = None) -> SegmentReport:
        """ccsx_segment_reads: k_segment on the caller's reads, a list of arrays of codes 0 .. 3 (an empty one is untested).  Synchronous; no slot is touched"""
        return self._reads(SegmentReport, sset, reads, opts, report)

    # ---- full-length cDNA reads (ccsx_consensus_cdna / ccsx_cdna_reads): primers, strand, poly(A) tail and concatemers of the final reads
    def consensus_cdna(self, batch: Batch, primers: CdnaPrimers, opts: "CdnaOpts | None" = None, res: "Results | None" = None,
                       **requests) -> tuple["Results", CdnaReport]:
        """(results, cdna report).  primers: the CdnaPrimers; opts: the CdnaOpts (None: the defaults); res: the caller's Results.  requests: Handle.submit's
        keyword arguments for the other requests of the same run (pileup=, tandem=, fold=, adapters=, control=, coverage= ... with their reports; not hd=,
        handoff=, barcodes=, represent=, segments=)"""
        return self._consensus_reads("cdna", CdnaReport, batch, primers, opts, res, requests)

    def cdna_reads(self, primers: CdnaPrimers, reads, opts: "CdnaOpts | None" = None, report: "CdnaReport | None" = None) -> CdnaReport:
        """ccsx_cdna_reads: k_cdna on the caller's reads, a list of arrays of codes 0 .. 3 (an empty one is untested).  Synchronous; no slot is touched"""
        return self._reads(CdnaReport, primers, reads, opts, report)

    # ---- cell barcodes and UMIs (ccsx_cell_reads): the cDNA analysis with the two fields behind one primer read, corrected against a whitelist and clipped
    def cell_reads(self, primers: CdnaPrimers, reads, design: "CellDesign | None" = None, whitelist: "CellWhitelist | None" = None, opts: "CdnaOpts | None" = None,
                   report: "CellReport | None" = None) -> CellReport:
        """ccsx_cell_reads: k_cell on the caller's reads, a list of arrays of codes 0 .. 3 (an empty one is untested).  Synchronous; no slot is touched.  The
        whitelist's table stays on the device until a call brings another one"""
        args, rep, _keep = _cell_reads_args(primers, opts, design, whitelist, reads, report)
        self._check(self._L.ccsx_cell_reads(self._h, *args), "ccsx_cell_reads")
        return rep

    # ---- duplicate reads (ccsx_dup_sign_reads / ccsx_dup_cluster): the sets of reads that are the same molecule
    def dup_sign(self, reads, opts: "DupOpts | None" = None) -> np.ndarray:
        """ccsx_dup_sign_reads: k_dup_sign on the caller's reads, a list of arrays of codes 0 .. 3: their signatures (DUP_SIG_DTYPE).  Synchronous; no slot is touched"""
        args, sig, _keep = _dup_sign_args(reads, opts)
        self._check(self._L.ccsx_dup_sign_reads(self._h, *args), "ccsx_dup_sign_reads")
        return sig

    def dup_cluster(self, sig, group=None, score=None, opts: "DupOpts | None" = None, report: "DupReport | None" = None) -> DupReport:
        """ccsx_dup_cluster: the duplicate sets of the signatures (group / score: None, or one int32 per read).  Synchronous; no slot is touched"""
        args, rep, _keep = _dup_cluster_args(sig, group, score, opts, report)
        self._check(self._L.ccsx_dup_cluster(self._h, *args), "ccsx_dup_cluster")
        return rep

    def mark_duplicates(self, reads, group=None, score=None, opts: "DupOpts | None" = None) -> DupReport:
        """dup_sign, then dup_cluster on its signatures"""
        return self.dup_cluster(self.dup_sign(reads, opts), group, score, opts)

    # ---- representative reads (ccsx_consensus_represent): a draft or a subread in the result planes of every ZMW that was not polished
    def consensus_represent(self, batch: Batch, subread_fallback: bool = False, kinetics: bool = False, res: "Results | None" = None,
                            **requests) -> tuple["Results", RepresentReport]:
        """(results, represent report).  subread_fallback: a ZMW that would get its draft gets a subread; kinetics: SUBREAD ZMWs get fi / fp (needs
        opts.hifi_kinetics and batch.ipd); res: the caller's Results.  requests: Handle.submit's keyword arguments for the other requests of the same run
        (pileup=, tandem=, fold=, adapters=, control=, coverage= without a gate ... with their reports; not hd=, handoff=, barcodes=)"""
        if res is None:
            res = Results.allocate(batch, kinetics=bool(self.opts.hifi_kinetics))
        rep = RepresentReport.allocate(batch.n_zmw)
        self._fused("consensus", batch, res, _requests(via_requests=True, **requests), represent=(rep, subread_fallback, kinetics))
        return res, rep

    def barcode_reads(self, bset: BarcodeSet, reads, opts: "BarcodeOpts | None" = None, report: "BarcodeReport | None" = None) -> BarcodeReport:
        """ccsx_barcode_reads: k_barcode on the caller's reads, a list of arrays of codes 0 .. 3 (an empty one is untested).  Synchronous; no slot is touched"""
        return self._reads(BarcodeReport, bset, reads, opts, report)

    # ---- the polisher hand-back (ccsx_refine_batch): refined tiles spliced into the base consensus on the GPU, QVs from one more Arrow round
    @staticmethod
    def _refine_args(batch: Batch, base: "Results", tiles: "RefineTiles", backbone, res: "Results", report: "RefineReport"):
        bb = np.ascontiguousarray(np.asarray(backbone, np.int32))
        if len(bb) != batch.n_zmw:
            raise ValueError("backbone: one int32 per ZMW")
        keep = (batch, base, tiles, bb, res, report, batch.c_struct(), base.c_struct(), tiles.c_struct(), res.c_struct(), report.c_struct())
        cb, cbase, ct, cr, crep = keep[6:]
        return (C.byref(cb), C.byref(cbase), _ptr(bb, C.c_int32), C.byref(ct), C.byref(cr), C.byref(crep)), keep

    def refine(self, batch: Batch, base: "Results", tiles: "RefineTiles", backbone, report: "RefineReport | None" = None) -> tuple["Results", "RefineReport"]:
        """(results, report).  base: the Results of an earlier run on `batch`; tiles: the RefineTiles; backbone: [n_zmw] a pass in SEQ's orientation per ZMW
        (Handoff.backbones; < 0 leaves the ZMW out).  The results are those of polish(batch, spliced drafts, QV_ONLY); rq_merged is in the report"""
        res = Results.allocate(batch, kinetics=bool(self.opts.hifi_kinetics))
        rep = report if report is not None else RefineReport.allocate(batch)
        args, _keep = self._refine_args(batch, base, tiles, backbone, res, rep)
        self._check(self._L.ccsx_refine_batch(self._h, *args), "ccsx_refine_batch")
        return res, rep

    def submit_refine(self, batch: Batch, base: "Results", tiles: "RefineTiles", backbone, res: "Results", report: "RefineReport") -> int:
        """the ticketed form (wait / release as for submit): every array belongs to the ticket until it is waited for"""
        args, keep = self._refine_args(batch, base, tiles, backbone, res, report)
        t = C.c_int64()
        self._check(self._L.ccsx_submit_refine(self._h, *args, C.byref(t)), "ccsx_submit_refine")
        if not hasattr(self, "_inflight"):
            self._inflight = {}
        self._inflight[t.value] = (batch, res, keep)
        return t.value

    def stage_polished(self, z: int):
        """after consensus_pileup: (templates [nw, 32] uint8, meta [nw, 3] int32 = J, cs, ce, passes used, backbone) of ZMW z's converged windows"""
        cap = 1 << 14
        tpl, meta = np.zeros(cap * 32, np.uint8), np.zeros(cap * 3, np.int32)
        nw, nr, bb = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._L.ccsx_stage_polished(self._h, z, _ptr(tpl, C.c_uint8), _ptr(meta, C.c_int32), cap, C.byref(nw), C.byref(nr), C.byref(bb)),
                    "ccsx_stage_polished")
        n = nw.value
        return tpl[: n * 32].reshape(n, 32).copy(), meta[: n * 3].reshape(n, 3).copy(), nr.value, bb.value

    def upload(self, batch: Batch):
        self._keep = batch
        cb = batch.c_struct()
        self._check(self._L.ccsx_upload(self._h, C.byref(cb)), "ccsx_upload")
        self._sync_reads = int(batch.read_off[-1])

    def run(self):
        self._check(self._L.ccsx_run(self._h), "ccsx_run")

    def sync(self):
        self._check(self._L.ccsx_sync(self._h), "ccsx_sync")

    def download(self) -> Results:
        res = Results.allocate(self._keep, kinetics=bool(self.opts.hifi_kinetics))
        cr = res.c_struct()
        self._check(self._L.ccsx_download(self._h, C.byref(cr)), "ccsx_download")
        return res

    def timings(self) -> Timings:
        t = Timings()
        self._check(self._L.ccsx_get_timings(self._h, C.byref(t)), "ccsx_get_timings")
        return t

    # ---- asynchronous pipeline (ccsx_submit / ccsx_wait): up to three batches in flight, copies under compute
    def submit(self, batch: Batch, res: "Results", pileup: "Pileup | None" = None, tandem: "np.ndarray | None" = None,
               min_tandem_repeat_length: int = 0, hd: "HdReport | None" = None, hd_opts: HdOpts | None = None, hd_split: bool = False,
               fold: "FoldReport | None" = None, fold_opts: FoldOpts | None = None, adapters: "AdapterReport | None" = None,
               adapter_set: "AdapterSet | None" = None, adapter_opts: "AdapterOpts | None" = None, control: "ControlReport | None" = None,
               control_seq: "ControlSeq | None" = None, control_opts: "ControlOpts | None" = None, coverage: "CoverageReport | None" = None,
               coverage_opts: "CoverageOpts | None" = None, coverage_gate: int = 0, handoff: "Handoff | None" = None,
               barcodes: "BarcodeReport | None" = None, barcode_set: "BarcodeSet | None" = None, barcode_opts: "BarcodeOpts | None" = None,
               represent: "RepresentReport | None" = None, represent_fallback: bool = False, represent_kinetics: bool = False,
               segments: "SegmentReport | None" = None, segment_set: "SegmentSet | None" = None, segment_opts: "SegmentOpts | None" = None,
               cdna: "CdnaReport | None" = None, cdna_primers: "CdnaPrimers | None" = None, cdna_opts: "CdnaOpts | None" = None) -> int:
        """pileup: also the pileup summary's planes, complete when the ticket is.  tandem: an int32 [n_zmw] array (tandem_buffer, pinned) that receives
        tandem_len; min_tandem_repeat_length > 0 switches the heuristics off for flagged ZMWs.  hd: a report (HdReport.allocate(n, pinned=True)) that
        receives the heteroduplex finder's verdicts, hd_split=True keeps HETERODUPLEX ZMWs out of the polish stage (ccsx_submit_hd; with fold, adapters, control
        or coverage in the same call: ccsx_submit_hd_requests, include/ccsx.h has the order in which the coverage gate and the split give a status).  fold: a report
        (FoldReport.allocate(n, pinned=True)) that receives the adapter-palindrome verdicts.  adapters: a report (AdapterReport.allocate(n, pinned=True))
        that receives the adapter screen of adapter_set (None: the built-in set) under adapter_opts.  control: a report (ControlReport.allocate(n,
        pinned=True)) that receives the control screen for control_seq under control_opts.  fold, adapters and control go alone or together
        (ccsx_submit_control).  Every ticket carries its own control: tickets in flight may screen for different ones.  coverage: a
        report (CoverageReport.allocate(n, pinned=True)) that receives the coverage screen under coverage_opts and coverage_gate (ccsx_submit_requests; with or
        without the other screens); every ticket carries its own options and gate.  handoff: a Handoff (Handoff.allocate(batch, max_tiles, opts,
        pinned=True) or device=) that receives the polisher hand-off (ccsx_submit_handoff; not with hd): the whole capacity of its arrays is copied, complete
        when the ticket is; every ticket carries its own options and capacity.  barcodes: a report (BarcodeReport.allocate(n, pinned=True)) that receives the
        barcode calls for barcode_set under barcode_opts (ccsx_submit_barcodes; not with hd or handoff); every ticket carries its own set and options.  represent: a report
        (RepresentReport.allocate(n, pinned=True)) that receives the representative classes; the ZMWs that were not polished get a draft or a subread in `res`
        (ccsx_submit_represent; represent_fallback / represent_kinetics: the request's flags, every ticket its own; not with hd, handoff, barcodes or a
        coverage gate).  segments: a report (SegmentReport.allocate(n, pinned=True)) that receives the segmentation for segment_set under segment_opts
        (ccsx_submit_segments; not with hd, handoff, barcodes or represent); every ticket carries its own set and options.  cdna: a report
        (CdnaReport.allocate(n, pinned=True)) that receives the cDNA analysis for cdna_primers under cdna_opts (ccsx_submit_cdna; not with hd, handoff, barcodes,
        represent or segments); every ticket carries its own set and options"""
        one = _exclusive(hd is not None, handoff, barcodes, represent, segments, cdna)   # (refused before anything else is looked at)
        if tandem is not None and (tandem.dtype != np.int32 or len(tandem) < batch.n_zmw or not tandem.flags.c_contiguous):
            raise ValueError("tandem: an int32 array of n_zmw elements (tandem_buffer)")
        if control is not None and control_seq is None:
            raise ValueError("control: a control_seq is needed (there is no built-in control)")
        requests = _requests(pileup, tandem, min_tandem_repeat_length, hd, hd_opts, hd_split, fold, fold_opts, adapters, adapter_set, adapter_opts,
                             control, control_seq, control_opts, coverage, coverage_opts, coverage_gate,
                             via_requests=one is not None, hd_requests=True)
        t = C.c_int64()
        cb, cr = self._fused("submit", batch, res, requests, t, handoff=handoff,
                             barcodes=(barcodes, barcode_set, barcode_opts) if barcodes is not None else None,
                             represent=(represent, represent_fallback, represent_kinetics) if represent is not None else None,
                             segments=(segments, segment_set, segment_opts) if segments is not None else None,
                             cdna=(cdna, cdna_primers, cdna_opts) if cdna is not None else None)
        if not hasattr(self, "_inflight"):
            self._inflight = {}
        self._inflight[t.value] = (batch, res, cb, cr, requests, handoff)  # the C structs and arrays must outlive the ticket
        return t.value

    def wait(self, ticket: int) -> "Results":
        self._check(self._L.ccsx_wait(self._h, ticket), "ccsx_wait")
        return self._inflight[ticket][1]

    def release(self, ticket: int):
        self._inflight.pop(ticket, None)

    def poll(self, ticket: int) -> bool:
        rc = self._L.ccsx_poll(self._h, ticket)
        if rc < 0:
            self._check(rc, "ccsx_poll")
        return rc == 1

    def ticket_timings(self, ticket: int) -> Timings:
        t = Timings()
        self._check(self._L.ccsx_ticket_timings(self._h, ticket, C.byref(t)), "ccsx_ticket_timings")
        return t

    def stage_draft(self, z: int) -> np.ndarray:
        cap = 1 << 17
        buf = np.zeros(cap, np.uint8)
        n = C.c_int32()
        self._check(self._L.ccsx_stage_draft(self._h, z, _ptr(buf, C.c_uint8), cap, C.byref(n)), "ccsx_stage_draft")
        return buf[: n.value].copy()

    def stage_align(self, r: int, ld: int):
        buf = np.zeros(ld + 1, np.int32)
        v, s = C.c_int32(), C.c_int32()
        self._check(self._L.ccsx_stage_align(self._h, r, _ptr(buf, C.c_int32), ld + 1, C.byref(v), C.byref(s)), "ccsx_stage_align")
        return buf, v.value, s.value

    def stage_align_ev(self, r: int, ld: int):
        """stage_align plus dirty[ld] (uint8): the pass's pile-up evidence per draft position, as k_polish reads it (all 1 for a split or partial pass)"""
        buf, dirty = np.zeros(ld + 1, np.int32), np.zeros(max(ld, 1), np.uint8)
        v, s = C.c_int32(), C.c_int32()
        self._check(self._L.ccsx_stage_align_ev(self._h, r, _ptr(buf, C.c_int32), ld + 1, C.byref(v), C.byref(s), _ptr(dirty, C.c_uint8), ld), "ccsx_stage_align_ev")
        return buf, v.value, s.value, dirty[:ld]

    def poa_log(self, on: bool = True):
        """ask for (or drop) the POA log: batches staged from now on keep one record per (ZMW, draft generator, pass); the layout is in
        include/ccsx.h under "The POA log" """
        self._check(self._L.ccsx_poa_log(self._h, int(bool(on))), "ccsx_poa_log")

    def stage_poa(self, z: int):
        """the POA log of ZMW z in the batch run last: per draft generator (0 = POA on pass 0, 1 = the fallback) an int32 array [k, 6] of the passes the
        generator's DP saw, one row (rr, I, end score, end position or -1, threaded 0/1, vertices after the pass) per pass, rr = 1 .. in order"""
        out = []
        for gen in (0, 1):
            buf, n = np.zeros((64, POA_LOG_WORDS), np.int32), C.c_int32(0)
            rc = self._L.ccsx_stage_poa(self._h, z, gen, _ptr(buf, C.c_int32), len(buf), C.byref(n))
            if rc != 0 and n.value > len(buf):           # refused for its size alone: the batch has a ZMW of more passes, n says how many
                buf = np.zeros((n.value, POA_LOG_WORDS), np.int32)
                rc = self._L.ccsx_stage_poa(self._h, z, gen, _ptr(buf, C.c_int32), len(buf), C.byref(n))
            self._check(rc, "ccsx_stage_poa")
            rr = [k for k in range(n.value) if buf[k, 0] >= 0]
            out.append(np.array([[k, *buf[k]] for k in rr], np.int32).reshape(len(rr), POA_LOG_WORDS + 1))
        return out

    def stage_windows(self, z: int) -> np.ndarray:
        cap = 1 << 14
        buf = np.zeros(cap, np.int32)
        n = C.c_int32()
        self._check(self._L.ccsx_stage_windows(self._h, z, _ptr(buf, C.c_int32), cap, C.byref(n)), "ccsx_stage_windows")
        return buf[: n.value + 1].copy()

    def stage_wmeta(self, z: int) -> np.ndarray:
        """what k_polish left per window of ZMW z: int32 [n_windows, 5] = (core length, usable reads of the last round over all passes, the same over the
        full-length passes only, non-convergent 0/1, scoring rounds)"""
        cap = 1 << 14
        buf = np.zeros((cap, 5), np.int32)
        n = C.c_int32()
        self._check(self._L.ccsx_stage_wmeta(self._h, z, _ptr(buf, C.c_int32), cap, C.byref(n)), "ccsx_stage_wmeta")
        return buf[: n.value].copy()

    def close(self):
        if self._h:
            self._L.ccsx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_count() -> int:
    return lib().ccsx_device_count()


def split_strands(batch: Batch, zmw_mask) -> tuple[Batch, np.ndarray, np.ndarray]:
    """the selected ZMWs as single-strand ZMWs: for each, its forward passes (flags bit 0 clear) as one ZMW, then its reverse passes as the next, both
    keeping zmw_id (the `ccs` driver's --by-strand split).  A strand without passes yields no ZMW.  Returns (batch, source ZMW index, strand 0/1) per new ZMW;
    partial passes stay behind the full-length passes of their strand."""
    sel = np.flatnonzero(np.asarray(zmw_mask, bool))
    read_off, base_off, reads, src, strand = [0], [0], [], [], []
    for z in sel:
        r0, r1 = int(batch.read_off[z]), int(batch.read_off[z + 1])
        for s in (0, 1):
            rr = [r for r in range(r0, r1) if (int(batch.flags[r]) & 1) == s]
            if not rr:
                continue
            rr = [r for r in rr if not batch.flags[r] & 2] + [r for r in rr if batch.flags[r] & 2]
            reads += rr; src.append(int(z)); strand.append(s)
            read_off.append(read_off[-1] + len(rr))
    reads = np.array(reads, np.int64)
    lens = (batch.base_off[reads + 1] - batch.base_off[reads]) if len(reads) else np.zeros(0, np.int64)
    base_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.concatenate([np.arange(batch.base_off[r], batch.base_off[r + 1]) for r in reads]) if len(reads) else np.zeros(0, np.int64)
    src = np.array(src, np.int64)
    out = Batch(np.ascontiguousarray(batch.zmw_id[src]), np.ascontiguousarray(batch.snr[src]), np.array(read_off, np.int32), base_off,
                np.ascontiguousarray(batch.bases[idx]), np.ascontiguousarray(batch.pw[idx]), np.ascontiguousarray(batch.ipd[idx]),
                np.ascontiguousarray(batch.flags[reads]))
    return out, src, np.array(strand, np.int8)


@dataclass
class HdRecord:
    """one read of the heteroduplex mode: the read group (DS = both strands, fwd / rev = one strand of a heteroduplex,
    docs/faq/mode-heteroduplex-filtering.md:44-51) and its consensus"""
    zmw: int
    zmw_id: int
    group: str
    status: int
    seq: np.ndarray
    qual: np.ndarray
    rq: float
    np_: int


def consensus_hd(handle: "Handle", batch: Batch, opts: HdOpts | None = None):
    """the heteroduplex mode end to end: draft -> hd -> polish of the same drafts -> consensus of the strands of every HETERODUPLEX.  Returns
    (records, report): one DS record per other ZMW (byte for byte what `consensus` gives), up to two (fwd, rev) per heteroduplex."""
    drafts = handle.draft(batch)
    rep = handle.hd(batch, drafts, opts)
    res = handle.polish(batch, drafts)
    het = rep.verdict == HD_HETERODUPLEX
    strands = {}
    if het.any():
        sb, src, strand = split_strands(batch, het)
        sres = handle.consensus(sb)
        for i in range(sb.n_zmw):
            strands[(int(src[i]), int(strand[i]))] = (sres, i)
    recs = []
    for z in range(batch.n_zmw):
        parts = [("fwd", strands.get((z, 0))), ("rev", strands.get((z, 1)))] if het[z] else [("DS", (res, z))]
        for group, got in parts:
            if got is None:
                continue
            r, i = got
            recs.append(HdRecord(z, int(batch.zmw_id[z]), group, int(r.status[i]), r.sequence(i).copy(), r.quals(i).copy(), float(r.rq[i]), int(r.np_[i])))
    return recs, rep


def _stream_requests(b: Batch, res: "Results", fold=False, adapter_set=None, adapter_opts=None, control_seq=None, control_opts=None, coverage=False,
                     coverage_gate=0, pileup=False, tandem=False, min_tandem_repeat_length=0) -> dict:
    """Handle.submit's keywords for one ticket of consensus_hd_stream: the requests as the stream was given them, with page-locked reports of this batch's size"""
    n, kw = b.n_zmw, dict(min_tandem_repeat_length=min_tandem_repeat_length)
    if pileup:
        kw["pileup"] = Pileup.allocate(res, pinned=True)
    if tandem:
        kw["tandem"] = tandem_buffer(n, pinned=True)
    if fold:
        kw.update(fold=FoldReport.allocate(n, pinned=True), fold_opts=fold if isinstance(fold, FoldOpts) else None)
    if adapter_set is not None:
        kw.update(adapters=AdapterReport.allocate(n, pinned=True), adapter_set=adapter_set, adapter_opts=adapter_opts)
    if control_seq is not None:
        kw.update(control=ControlReport.allocate(n, pinned=True), control_seq=control_seq, control_opts=control_opts)
    if coverage:
        kw.update(coverage=CoverageReport.allocate(n, pinned=True), coverage_opts=coverage if isinstance(coverage, CoverageOpts) else None,
                  coverage_gate=coverage_gate)
    return kw


def consensus_hd_stream(handle: "Handle", batches, opts: HdOpts | None = None, tickets_out: "list | None" = None, **requests):
    """the heteroduplex mode, pipelined: every batch goes through ONE ticket with the finder and the split (ccsx_submit_hd, split = 1), and when that ticket
    is retired its HETERODUPLEX ZMWs become a single-strand batch (split_strands) for an ordinary ticket.  At most three tickets are in flight (the handle's
    slots); yields (records, report) per input batch, in input order, with exactly the records consensus_hd gives.
    requests: fold= (True or a FoldOpts), adapter_set= / adapter_opts=, control_seq= / control_opts=, coverage= (True or a CoverageOpts) / coverage_gate=,
    pileup=, tandem=, min_tandem_repeat_length= go into every ticket (ccsx_submit_hd_requests); the strand ticket carries the same requests without the finder.
    tickets_out: a list that receives (input index, "hd" or "strand", batch, results, Handle.submit's keywords with the reports) per retired ticket."""
    from collections import deque
    inflight = deque()                 # (ticket, input index, kind): retired oldest first, so the in-flight tickets are always the latest submitted
    state, done, nxt = {}, {}, 0

    def finish(i, sres=None, src=None, strand=None):
        b, res, rep = state[i]["batch"], state[i]["res"], state[i]["rep"]
        het = rep.verdict == HD_HETERODUPLEX
        strands = {}
        if sres is not None:
            for k in range(len(src)):
                strands[(int(src[k]), int(strand[k]))] = (sres, k)
        recs = []
        for z in range(b.n_zmw):
            parts = [("fwd", strands.get((z, 0))), ("rev", strands.get((z, 1)))] if het[z] else [("DS", (res, z))]
            for group, got in parts:
                if got is None:
                    continue
                r, k = got
                recs.append(HdRecord(z, int(b.zmw_id[z]), group, int(r.status[k]), r.sequence(k).copy(), r.quals(k).copy(), float(r.rq[k]), int(r.np_[k])))
        done[i] = (recs, rep)
        del state[i]

    def retire_oldest():
        t, i, kind = inflight.popleft()
        handle.wait(t)
        handle.release(t)
        if tickets_out is not None:
            st = state[i]
            tickets_out.append((i, kind, st["sb"], st["sres"], st["skw"]) if kind == "strand" else (i, kind, st["batch"], st["res"], st["kw"]))
        if kind == "strand":
            st = state[i]
            finish(i, st["sres"], st["src"], st["strand"])
            return
        het = state[i]["rep"].verdict == HD_HETERODUPLEX
        if not het.any():
            finish(i)
            return
        sb, src, strand = split_strands(state[i]["batch"], het)
        sres = Results.allocate(sb, kinetics=bool(handle.opts.hifi_kinetics), pinned=True)
        skw = _stream_requests(sb, sres, **requests)
        state[i].update(sb=sb, sres=sres, src=src, strand=strand, skw=skw)
        inflight.append((handle.submit(sb, sres, **skw), i, "strand"))      # (one ticket was just retired: at most three in flight)

    for i, b in enumerate(batches):
        while len(inflight) >= 3:
            retire_oldest()
        res = Results.allocate(b, kinetics=bool(handle.opts.hifi_kinetics), pinned=True)
        rep = HdReport.allocate(b.n_zmw, pinned=True)
        kw = _stream_requests(b, res, **requests)
        state[i] = dict(batch=b, res=res, rep=rep, kw=kw)
        inflight.append((handle.submit(b, res, hd=rep, hd_opts=opts, hd_split=True, **kw), i, "hd"))
        while nxt in done:
            yield done.pop(nxt)
            nxt += 1
    while inflight:
        retire_oldest()
        while nxt in done:
            yield done.pop(nxt)
            nxt += 1


# ---- BGZF inflate (include/ccsx.h "BGZF inflate on the device"; DESIGN.md §2 "BGZF inflate")
INFLATE_MAX_OUT = 65536
INFLATE_STATUS_NAMES = ["OK", "TRUNCATED_INPUT", "BAD_BLOCK_TYPE", "BAD_STORED_LENGTH", "BAD_CODE_LENGTHS", "BAD_SYMBOL", "BAD_DISTANCE", "OUTPUT_OVERRUN",
                        "OUTPUT_SHORT"]


def bgzf_split(data: bytes) -> list:
    """The blocks of a BGZF byte string as (payload, isize, crc32): payload = the raw DEFLATE stream between the gzip member's header and its 8-byte trailer"""
    out, at = [], 0
    while at < len(data):
        if len(data) - at < 18 or data[at:at + 2] != b"\x1f\x8b" or not data[at + 3] & 4:
            raise ValueError(f"not a BGZF block at byte {at}")
        xlen = int.from_bytes(data[at + 10:at + 12], "little")
        bsize, p = 0, at + 12
        while p + 4 <= at + 12 + xlen:
            sl = int.from_bytes(data[p + 2:p + 4], "little")
            if data[p:p + 2] == b"BC" and p + 6 <= at + 12 + xlen:
                bsize = int.from_bytes(data[p + 4:p + 6], "little") + 1
            p += 4 + sl
        if not bsize or bsize < 12 + xlen + 8 or at + bsize > len(data):
            raise ValueError(f"truncated or malformed BGZF block at byte {at}")
        end = at + bsize
        out.append((data[at + 12 + xlen:end - 8], int.from_bytes(data[end - 4:end], "little"), int.from_bytes(data[end - 8:end - 4], "little")))
        at = end
    return out


class _CodecCall:
    """The buffers of one codec call: inputs packed back to back (gap bytes apart) in src, output ranges of range_lens[i] bytes packed (guard bytes before,
    between and behind them) in dst, the list items (of the subclass's ITEM type: in_off, in_len, the range's length, out_off) and the status array"""
    ITEM = None

    def __init__(self, inputs, range_lens, guard: int = 0, gap: int = 0, fill: int = 0):
        n = len(inputs)
        assert n == len(range_lens)
        self.items = (self.ITEM * max(n, 1))()
        src, ioff, ooff = bytearray(), 0, guard
        for i, (p, ol) in enumerate(zip(inputs, range_lens)):
            self.items[i] = self.ITEM(ioff, len(p), int(ol), ooff)
            src += p + b"\0" * gap
            ioff += len(p) + gap
            ooff += int(ol) + guard
        self.n, self.guard = n, guard
        self.src = np.frombuffer(bytes(src) or b"\0", dtype=np.uint8).copy()
        self.src_len = len(src)
        self.dst = np.full(max(ooff, 1), fill, dtype=np.uint8)
        self.dst_len = ooff
        self.status = np.full(max(n, 1), -1, dtype=np.int32)

    def _results(self):
        """the result arrays as the entry points take them"""
        return (_ptr(self.status, C.c_int32),)

    def args(self):
        return (_ptr(self.src, C.c_uint8), self.src_len, self.items, self.n, _ptr(self.dst, C.c_uint8), self.dst_len, *self._results())


class InflateCall(_CodecCall):
    """The buffers of one inflate call: payloads packed back to back (gap bytes apart) in src, outputs packed (guard bytes before, between and behind them) in dst"""
    ITEM = DeflateBlock

    def __init__(self, payloads, out_lens, guard: int = 0, gap: int = 0, fill: int = 0):
        super().__init__(payloads, out_lens, guard, gap, fill)
        self.blocks = self.items

    def output(self, i: int) -> bytes:
        b = self.blocks[i]
        return self.dst[b.out_off:b.out_off + b.out_len].tobytes()

    def outputs(self) -> bytes:
        return b"".join(self.output(i) for i in range(self.n))


def _codec_host(fn: str, call: _CodecCall):
    if getattr(lib(), fn)(*call.args()) != 0:
        raise RuntimeError(fn + " failed: " + lib().ccsx_last_error().decode())
    return call.status[:call.n].copy(), call


def inflate_host(payloads, out_lens, **layout):
    """ccsx_inflate_blocks_host: the decoder of k_inflate on the calling thread, no device.  Returns (the outputs concatenated, status array, the call)"""
    status, call = _codec_host("ccsx_inflate_blocks_host", InflateCall(payloads, out_lens, **layout))
    return call.outputs(), status, call


class _Codec:
    """One codec object bound to one GPU: its own stream and buffers.  The subclass names its entry points (CREATE, DESTROY, SUBMIT, WAIT, RUN).  Not thread-safe."""
    CREATE = DESTROY = SUBMIT = WAIT = RUN = ""

    def __init__(self, device: int, max_in_bytes: int, max_out_bytes: int, max_items: int):
        self._L = lib()
        self._f = C.c_void_p()
        self.max_in_bytes, self.max_out_bytes = max_in_bytes, max_out_bytes
        self._check(getattr(self._L, self.CREATE)(device, max_in_bytes, max_out_bytes, max_items, C.byref(self._f)), self.CREATE)
        self._calls = {}

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed: " + self._L.ccsx_last_error().decode())

    def submit(self, call) -> int:
        t = C.c_int64()
        self._check(getattr(self._L, self.SUBMIT)(self._f, *call.args(), C.byref(t)), self.SUBMIT)
        self._calls[t.value] = call      # the call's arrays stay alive until the ticket is waited for
        return t.value

    def wait(self, ticket: int):
        self._check(getattr(self._L, self.WAIT)(self._f, ticket), self.WAIT)
        return self._calls.pop(ticket)

    def run(self, call):
        self._check(getattr(self._L, self.RUN)(self._f, *call.args()), self.RUN)
        return call

    def close(self):
        if self._f:
            getattr(self._L, self.DESTROY)(self._f)
            self._f = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Inflater(_Codec):
    """One BGZF inflater bound to one GPU (ccsx_inflater_create): its own stream and buffers, nothing shared with a Handle.  Not thread-safe."""
    CREATE, DESTROY, SUBMIT, WAIT, RUN = "ccsx_inflater_create", "ccsx_inflater_destroy", "ccsx_inflate_submit", "ccsx_inflate_wait", "ccsx_inflate_blocks"

    def __init__(self, device: int = 0, max_in_bytes: int = 1 << 21, max_out_bytes: int = 1 << 23, max_blocks: int = 256):
        self.max_blocks = max_blocks
        super().__init__(device, max_in_bytes, max_out_bytes, max_blocks)

    def inflate(self, blocks, out_lens):
        """blocks: raw DEFLATE payloads; out_lens: the bytes each inflates to.  Returns (the outputs concatenated, status array); the bytes of a block whose
        status is not OK are unspecified"""
        call = self.run(InflateCall(blocks, out_lens))
        return call.outputs(), call.status[:call.n].copy()


# ---- BGZF deflate (include/ccsx.h "BGZF deflate on the device"; DESIGN.md §2 "BGZF deflate")
DEFLATE_MAX_IN = 65536
DEFLATE_STATUS_NAMES = ["OK", "OUTPUT_FULL"]


def deflate_bound(in_len: int) -> int:
    return int(lib().ccsx_deflate_bound(int(in_len)))


def deflate_crc(data: bytes) -> int:
    """ccsx_deflate_crc: the rule's sliced CRC32 alone, on the host"""
    a = np.frombuffer(bytes(data) or b"\0", dtype=np.uint8)
    return int(lib().ccsx_deflate_crc(_ptr(a, C.c_uint8), len(data)))


def deflate_code_lengths(freq, max_bits: int = 15) -> np.ndarray:
    """ccsx_deflate_code_lengths: the rule's length-limited code lengths for these symbol counts (host)"""
    f = np.ascontiguousarray(freq, dtype=np.uint32)
    lens = np.zeros(len(f), dtype=np.uint8)
    if lib().ccsx_deflate_code_lengths(_ptr(f, C.c_uint32), len(f), max_bits, _ptr(lens, C.c_uint8)) != 0:
        raise RuntimeError("ccsx_deflate_code_lengths failed: " + lib().ccsx_last_error().decode())
    return lens


class DeflateCall(_CodecCall):
    """The buffers of one deflate call: spans packed back to back (gap bytes apart) in src, output ranges of out_caps[i] bytes (default: the bound) packed
    (guard bytes before, between and behind them) in dst"""
    ITEM = DeflateSpan

    def __init__(self, spans, out_caps=None, guard: int = 0, gap: int = 0, fill: int = 0):
        super().__init__(spans, [deflate_bound(len(p)) for p in spans] if out_caps is None else out_caps, guard, gap, fill)
        self.spans = self.items
        self.out_len = np.full(max(self.n, 1), -1, dtype=np.int32)
        self.crc = np.zeros(max(self.n, 1), dtype=np.uint32)

    def _results(self):
        return (_ptr(self.out_len, C.c_int32), _ptr(self.crc, C.c_uint32), _ptr(self.status, C.c_int32))

    def stream(self, i: int) -> bytes:
        b = self.spans[i]
        return self.dst[b.out_off:b.out_off + int(self.out_len[i])].tobytes()

    def streams(self) -> list:
        return [self.stream(i) for i in range(self.n)]


def deflate_host(spans, out_caps=None, **layout):
    """ccsx_deflate_spans_host: the encoder of k_deflate on the calling thread, no device.  Returns (the streams, status array, the call)"""
    status, call = _codec_host("ccsx_deflate_spans_host", DeflateCall(spans, out_caps, **layout))
    return call.streams(), status, call


class Deflater(_Codec):
    """One BGZF deflater bound to one GPU (ccsx_deflater_create): its own stream and buffers, nothing shared with a Handle or an Inflater.  Not thread-safe."""
    CREATE, DESTROY, SUBMIT, WAIT, RUN = "ccsx_deflater_create", "ccsx_deflater_destroy", "ccsx_deflate_submit", "ccsx_deflate_wait", "ccsx_deflate_spans"

    def __init__(self, device: int = 0, max_in_bytes: int = 1 << 23, max_out_bytes: int = 1 << 23, max_spans: int = 256):
        self.max_spans = max_spans
        super().__init__(device, max_in_bytes, max_out_bytes, max_spans)

    def deflate(self, spans):
        """spans: plain byte strings of at most DEFLATE_MAX_IN bytes.  Returns (the streams, the CRC32s, status array)"""
        call = self.run(DeflateCall(spans))
        return call.streams(), call.crc[:call.n].copy(), call.status[:call.n].copy()
