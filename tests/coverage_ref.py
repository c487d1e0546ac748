"""The coverage rule (DESIGN.md §2 "Coverage rule", include/ccsx.h ccsx_coverage_*) in plain numpy: the reference of k_coverage / k_coverage_post.

Inputs are what the stage accessors (Handle.stage_windows / stage_align) and the CPU restatement (oracle_lib.windows / route) give: the draft's length, its
window bounds, and per pass (rstart by draft column, valid, length, is_partial).  Integer arithmetic only."""
import numpy as np

UNTESTED, NONE, DRAFT_TOO_DIFFERENT, INSUFFICIENT_SPANS, COVERAGE_DROPS, READS_FAILED_POLISHING = range(6)
PRE = ("verdict", "np_aligned", "spans", "cov_max", "clean_min", "drop_window", "drop_windows")
POST = ("reach_sum", "used_sum", "used_min")
FIELDS = PRE + POST
DEFAULTS = dict(drop_percent=50, block=30, min_spans=0, max_lost_percent=50)
OVERHANG = 2
SUCCESS, LOW_RQ = 0, 7                                   # enum ccsx_status: the final statuses READS_FAILED_POLISHING is decided for
GATE_STATUS = {DRAFT_TOO_DIFFERENT: 11, INSUFFICIENT_SPANS: 12, COVERAGE_DROPS: 13, READS_FAILED_POLISHING: 14}


def options(o=None):
    d = dict(DEFAULTS)
    d.update(o or {})
    return d


def edge_cols(bounds, Ld):
    """the draft columns of the 2 nw window-edge entries: 0, b1 - 2, b1 + 2, ..., Ld"""
    cols = [0] + [int(b) + s for b in bounds[1:-1] for s in (-OVERHANG, OVERHANG)] + [int(Ld)]
    assert all(a < b for a, b in zip(cols, cols[1:])), cols
    return cols


def windows(Ld, bounds, passes, block):
    """(reach_w, long_w, miss[r][w]) over the nw windows.  passes: (rstart, valid, length, is_partial) each"""
    nw = len(bounds) - 1
    cols = edge_cols(bounds, Ld)
    reach, lng = np.zeros(nw, np.int64), np.zeros(nw, np.int64)
    reaches = np.zeros((len(passes), nw), bool)
    for w in range(nw):
        ws, we = max(int(bounds[w]) - OVERHANG, 0), min(int(bounds[w + 1]) + OVERHANG, int(Ld))
        J = we - ws
        idx_ws = 2 * w - 1 if w else 0
        idx_we = 2 * nw - 1 if w == nw - 1 else 2 * (w + 1)
        for r, (rs, valid, L, _) in enumerate(passes):
            if not valid:
                continue
            n = int(rs[cols[idx_we]]) - int(rs[cols[idx_ws]])
            if 0 <= n <= int(L):
                reaches[r, w] = True
                reach[w] += 1
                lng[w] += n > J + block
    return reach, lng, reaches


def screen(Ld, bounds, passes, opts=None, min_passes=3, tested=True, used=None, final_status=SUCCESS, gate=0):
    """one ZMW's report as a dict over FIELDS.  tested: the status after the cascade is SUCCESS.  used: per window the passes the polish used (wmeta.y & 255),
    None when the ZMW was not polished (or the post-polish planes are not wanted): used_sum = used_min = 0 then and READS_FAILED_POLISHING is not reached.
    gate: a ZMW whose pre-polish verdict's bit is set was not polished, whatever `used` says"""
    o = options(opts)
    if not tested:
        return dict.fromkeys(FIELDS, 0)
    nw = len(bounds) - 1
    reach, lng, reaches = windows(Ld, bounds, passes, o["block"])
    clean = reach - lng
    full = [r for r, p in enumerate(passes) if p[1] and not p[3]]
    np_aligned = len(full)
    spans = sum(bool(reaches[r].all()) for r in full)
    cov_max = int(reach.max()) if nw else 0
    clean_min = int(clean.min()) if nw else 0
    drop_window = int(np.argmax(clean == clean_min)) if nw else 0          # the FIRST window with the fewest clean passes
    drop_windows = int((clean * 100 <= o["drop_percent"] * cov_max).sum())
    min_spans = o["min_spans"] or min_passes
    verdict = (DRAFT_TOO_DIFFERENT if np_aligned < min_passes else INSUFFICIENT_SPANS if spans < min_spans else COVERAGE_DROPS if drop_windows >= 1 else NONE)
    reach_sum, used_sum, used_min = int(reach.sum()), 0, 0
    if verdict != NONE and (gate >> verdict) & 1:
        used = None
    if used is not None:
        used = np.asarray(used, np.int64)
        assert len(used) == nw
        used_sum, used_min = int(used.sum()), int(used.min()) if nw else 0
        if verdict == NONE and final_status in (SUCCESS, LOW_RQ) and (reach_sum - used_sum) * 100 > o["max_lost_percent"] * reach_sum:
            verdict = READS_FAILED_POLISHING
    return dict(verdict=verdict, np_aligned=np_aligned, spans=spans, cov_max=cov_max, clean_min=clean_min, drop_window=drop_window, drop_windows=drop_windows,
                reach_sum=reach_sum, used_sum=used_sum, used_min=used_min)
