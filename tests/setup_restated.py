"""numpy restatements of what the layout build decides (pdlp_host.cpp / pdlp_solver.cpp on the host, pdlp_setup.hip /
k_block_span on the device), for tests/test_setup_cases_host.py and tests/test_gpu_setup_cases.py.  The partition and the
cold counts are those of tests/test_host.py."""
import numpy as np

from test_host import _cold_counts, _slab_partition_restated  # noqa: F401  (re-exported)

LONG_LIMIT = 256
MAJOR_COST = (2, 10)  # operand by rows, transposed operand (pdlp_host.hpp kSlabMajorCostRows / Cols)


def partition(beg, idx, n_major, n_minor, which, cold=True):
    """(n_blocks, minor_bits, wave_beg, cold counts) of operand `which`; cold = False: the same rule with no cold entry."""
    c = _cold_counts(beg, idx, n_minor, LONG_LIMIT) if cold else np.zeros(n_major, np.int64)
    nb, mb, wb = _slab_partition_restated(np.asarray(beg, np.int64), n_major, n_minor, LONG_LIMIT, MAJOR_COST[which], c)
    return nb, mb, wb, c


def xcd_of_block(b, nb):
    """pdlp_host.hpp xcdOfLogicalBlock: XCD x runs the logical blocks [x nb / 8, (x + 1) nb / 8), the first nb % 8 one more."""
    qlo, r = nb // 8, nb % 8
    if b < r * (qlo + 1):
        return b // (qlo + 1)
    return r + (b - r * (qlo + 1)) // qlo if qlo > 0 else 0


def tile_log2(n_minor):
    return max(14, int(np.ceil(np.log2(max(n_minor, 1)))) - 12)


def block_spans(beg, idx, wave_beg, n_minor):
    """Per block: first minor of its first-entry minimum, last-entry maximum and entry count over its SHORT non-empty majors
    (lo = INT32_MAX, hi = -1 where it has none); the [8, n_tiles] histogram of their entries per (XCD, tile)."""
    beg, idx = np.asarray(beg, np.int64), np.asarray(idx, np.int64)
    blk = np.asarray(wave_beg)[::16]
    nb = len(blk) - 1
    tl = tile_log2(n_minor)
    nt = ((max(n_minor, 1) - 1) >> tl) + 1
    lo, hi, cnt = np.full(nb, 2**31 - 1, np.int64), np.full(nb, -1, np.int64), np.zeros(nb, np.int64)
    hist = np.zeros((8, nt), np.int64)
    lens = np.diff(beg)
    for b in range(nb):
        r = np.arange(blk[b], blk[b + 1])
        r = r[(lens[r] > 0) & (lens[r] <= LONG_LIMIT)]
        if len(r) == 0:
            continue
        lo[b], hi[b], cnt[b] = idx[beg[r]].min(), idx[beg[r + 1] - 1].max(), lens[r].sum()
        ent = np.concatenate([idx[beg[k]:beg[k + 1]] for k in r])
        hist[xcd_of_block(b, nb)] += np.bincount(ent >> tl, minlength=nt)
    return lo, hi, cnt, hist, tl


def tile_owners(hist):
    """pdlp_host.cpp xcdTileOwners: (owner per tile, rule per tile) — rule "own": the XCD with the most entries there (the lowest
    on a tie); "left": the nearest owned tile to the left; "right": no owned tile to the left, the nearest to the right."""
    nt = hist.shape[1]
    own = [int(np.argmax(hist[:, t])) if hist[:, t].max() > 0 else -1 for t in range(nt)]
    rule = ["own" if o >= 0 else None for o in own]
    last = -1
    for t in range(nt):
        if own[t] >= 0:
            last = own[t]
        elif last >= 0:
            own[t], rule[t] = last, "left"
    last = -1
    for t in range(nt - 1, -1, -1):
        if rule[t] is not None:
            last = own[t]
        elif last >= 0:
            own[t], rule[t] = last, "right"
    for t in range(nt):
        if rule[t] is None:
            own[t], rule[t] = (t * 8) // nt, "proportional"
    return np.array(own, np.int64), rule


def few_tiles_margin(lo, hi, cnt):
    """DeviceMatrix::touchesFewTiles as the integer good * 5 - all * 4 (>= 0: slabs of 2^14 minors) and `all`."""
    good = tot = 0
    for l, h, c in zip(lo.tolist(), hi.tolist(), cnt.tolist()):
        if c <= 0:
            continue
        t = (h >> 14) - (l >> 14) + 1
        tot += c
        if t <= 8 and c * 8 >= t * (1 << 14):
            good += c
    return good * 5 - tot * 4, tot


def slab_width(lo, hi, cnt, forced=0):
    margin, tot = few_tiles_margin(lo, hi, cnt)
    return forced if forced > 0 else (14 if tot > 0 and margin >= 0 else 17)


def slab_layout(beg, idx, val, n_major, n_minor, wave_beg, minor_bits, W):
    """pdlp_host.cpp buildSlabLayout at slab width 2^W: long mask, long map, the long majors' compact CSR, wave_ptr, ent,
    val — a wave's short entries sorted by (minor >> W, major, minor)."""
    beg, idx, val = np.asarray(beg, np.int64), np.asarray(idx, np.int64), np.asarray(val, np.float64)
    wb = np.asarray(wave_beg, np.int64)
    lens = np.diff(beg)
    long_map = np.nonzero(lens > LONG_LIMIT)[0]
    mask = np.zeros((n_major + 31) // 32 + 1, np.uint32)
    np.bitwise_or.at(mask, long_map >> 5, (np.uint32(1) << (long_map & 31).astype(np.uint32)))
    pick = np.concatenate([np.arange(beg[r], beg[r + 1]) for r in long_map] + [np.zeros(0, np.int64)]).astype(np.int64)
    long_beg = np.concatenate([[0], np.cumsum(lens[long_map])])
    major = np.repeat(np.arange(n_major), lens)
    short = lens[major] <= LONG_LIMIT
    wave_of = np.searchsorted(wb, np.arange(n_major), side="right") - 1  # the LAST wave whose first major is <= r
    p = np.nonzero(short)[0]
    order = p[np.lexsort((idx[p], major[p], idx[p] >> W, wave_of[major[p]]))]
    w = wave_of[major[order]]
    wave_ptr = np.searchsorted(w, np.arange(len(wb)), side="left")
    ent = ((major[order] - wb[w]) << minor_bits) | idx[order]
    return dict(long_mask=mask, long_map=long_map, long_beg=long_beg, long_idx=idx[pick], long_val=val[pick], wave_ptr=wave_ptr,
                ent=ent.astype(np.uint32), slab_val=val[order], nnz_short=len(order))
