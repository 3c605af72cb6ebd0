"""The plan of the bucket MSM, restated (scroll-prover_amd/csrc/msm_plan.hpp): the window search, the plan of one pass, the batch splitter, the pipelined chunk count and
the host slice cuts, with the defaults of csrc/knobs.hpp.  A retune of the library changes THIS module; the lengths of tests/test_gpu_msm_plan_sweep.py follow from it, and
tests/test_msm_plan_on_host.py compares every field with the C++ planner on the CPU.  No GPU, no library: plain integers and IEEE doubles in the order the C++ writes them."""
SCALAR_BITS, AUTO_MAX_C, SORT_FB, RECORD_BYTES, L1_TILE = 255, 22, 11, 144, 16384
TAIL_COOP_MAX, FIXUP_LANES_MAX_LOG, REDUCE_CHAINS, REDUCE_MIN_CHUNK = 65536, 17, 131072, 4
G2_RECORD_BYTES, SORT_MAX_BINS, FIXUP_HUGE_MIN = 256, 4096, 2048
# csrc/knobs.hpp by environment name (the planner reads no other), the pipeline threshold of mi355_msm_set_pipeline, the calling thread's options and the CU count
DEFAULTS = {
    "MI355_SORT_FB": SORT_FB, "MI355_SORT_SPLIT": 1, "MI355_SORT_T1": L1_TILE, "MI355_SORT_T2": 0, "MI355_SEG_FACTOR": 16, "MI355_SEG_MIN": 16, "MI355_SEG_FILL": 40,
    "MI355_SEG_FILL_SEGFIX": 40, "MI355_FIXUP_MODE": 2, "MI355_FIXUP_SERIAL_MAX": 32, "MI355_FIXUP_HUGE_MIN": 2048, "MI355_FIXUP_LANES_MAX_LOG": FIXUP_LANES_MAX_LOG,
    "MI355_TAIL_COOP_MASK": 15, "MI355_TAIL_COOP_MAX": TAIL_COOP_MAX, "MI355_REDUCE_CHAINS": REDUCE_CHAINS, "MI355_REDUCE_MIN_CHUNK": REDUCE_MIN_CHUNK,
    "MI355_MSM_CHUNKS": 1, "MI355_HOST_CHUNKS": 8, "MI355_HOST_SLICE_MIN_LOG": 22, "MI355_MSM_AUTO_MAX_C": AUTO_MAX_C,
    "chunk_min_log": 23, "force_c": 0, "no_tables": 0, "cus": 256,
}
REFUSALS = {
    "entries": "msm: n * windows must be < 2^32", "buckets": "msm: too many buckets (split the batch)",
    "coarse": "msm: batch too large for the coarse histogram (split the batch)", "sorter": "msm: window bits out of range for the sorter",
}


def windows(c):
    return (SCALAR_BITS + c - 1) // c


def log2_ceil(n):
    return (n - 1).bit_length()


def ceil_div(a, b):
    return ((a + b - 1) // b) & 0xFFFFFFFF


def msm_cost(n, c, shared):
    """in units of one bucket addition: the entries' share, the bucket reduction, the Horner tail a table-free MSM waits for"""
    W, nb = float(windows(c)), float(1 << (c - 1))
    return 1.18 * W * float(n) + 8.2 * nb * (1.0 if shared else W) + (0.0 if shared else 3.0e7)


def best_window(n, max_c, shared):
    """the window search: the cheapest c in [4, max_c]; per-window bucket sets above 6 GB of G1 records are skipped"""
    best, best_c = 1e300, 8
    for c in range(4, max_c + 1):
        if not shared and windows(c) * float(1 << (c - 1)) * RECORD_BYTES > 6.0e9:
            continue
        cost = msm_cost(n, c, shared)
        if cost < best:
            best, best_c = cost, c
    return best_c


def choose_c(n, max_c=AUTO_MAX_C):
    return best_window(n, max_c, False)


def table_c(n_hint, max_c=AUTO_MAX_C):
    """mi355_srs_precompute(handle, 0, 0): the cheapest shared-bucket window for MSMs of n_hint points"""
    return best_window(n_hint, max_c, True)


def tables_close_enough(n, have_c, best_c):
    """mi355_srs_precompute's automatic choice keeps existing tables within 10 % of the best schedule"""
    return msm_cost(n, have_c, True) <= 1.10 * msm_cost(n, best_c, True)


def plan(n, M=1, tab_c=None, rec_bytes=RECORD_BYTES, forced=None, **settings):
    """plan_pass for M polynomials of n scalars.  tab_c: the window of the basis' tables (None: no tables); rec_bytes: 144 (G1) or 256 (G2: always the segmented fix-up
    at 100 % fill); forced: (c, shared) of another length (host slices); settings: entries of DEFAULTS to override.
    "fixup" is the form the per-bucket kernel has at this bucket count, "fixup_kind" what the pass runs ("segmented" where the segmented reduction replaces it)."""
    k = dict(DEFAULTS, **settings)
    assert set(k) == set(DEFAULTS), set(k) - set(DEFAULTS)
    g2 = rec_bytes == G2_RECORD_BYTES
    if forced:
        c, shared = forced
    else:
        c, shared = k["force_c"] or choose_c(n, k["MI355_MSM_AUTO_MAX_C"]), False
        if (tab_c and not k["force_c"] and not k["no_tables"] and msm_cost(n, tab_c, True) <= msm_cost(n, c, False)
                and (windows(tab_c) << log2_ceil(n)) < (1 << 31)):
            c, shared = tab_c, True
    W, kb = windows(c), c - 1
    entries = M * n * W
    fb = min(kb, k["MI355_SORT_FB"])
    if kb - fb > 11:
        fb = kb - 11
    cb_bits = kb - fb
    sets = M * (1 if shared else W)
    buckets = sets << kb
    regions = sets << cb_bits
    p = {"n": n, "M": M, "c": c, "W": W, "entries": entries, "shared": shared, "fb": fb, "cb_bits": cb_bits, "buckets": buckets, "regions": min(regions, 0xFFFFFFFF)}
    p["refusal"] = (REFUSALS["entries"] if entries >= 1 << 32 else REFUSALS["buckets"] if buckets >= 1 << 31 else REFUSALS["coarse"] if regions * 4 > 48 * 1024
                    else REFUSALS["sorter"] if fb > 12 or (1 << cb_bits) > SORT_MAX_BINS else None)
    p["must_split"] = p["refusal"] is not None or entries > 1 << 29 or buckets * rec_bytes > 8 << 30
    if p["refusal"]:
        return p
    # the accumulate launch
    want_threads = k["cus"] * 256 * k["MI355_SEG_FACTOR"]
    seg = min(max((entries + want_threads - 1) // want_threads, 16), 4096)
    blocks = ceil_div(ceil_div(entries, seg), 256)
    tn = blocks * 256
    segfix = g2 or k["MI355_FIXUP_MODE"] == 1 or (k["MI355_FIXUP_MODE"] == 2 and buckets >= 1 << 19 and seg * buckets >= entries)
    fill = 100 if g2 else k["MI355_SEG_FILL_SEGFIX"] if segfix else k["MI355_SEG_FILL"]
    seg_arg = seg | (min(k["MI355_SEG_MIN"], seg) << 13) | ((fill // 2) << 26)
    fixup = ("quad" if buckets * 4 <= k["MI355_TAIL_COOP_MAX"] and k["MI355_TAIL_COOP_MASK"] & 1 else
             "four lanes" if buckets <= (1 << k["MI355_FIXUP_LANES_MAX_LOG"]) else "one lane")
    p.update(seg=seg, blocks=blocks, tn=tn, seg_arg=seg_arg, fixup=fixup, fixup_kind="segmented" if segfix else fixup,
             big_cap=tn // k["MI355_FIXUP_SERIAL_MAX"] + 2, huge_cap=tn // FIXUP_HUGE_MIN + 2)
    # the sorter's tiles
    t1 = k["MI355_SORT_T1"]
    if k["MI355_SORT_SPLIT"] == 1 and t1 == 16384 and (1 << cb_bits) <= 1024 and entries >= 1 << 24:
        t1 = 24576
    t2 = k["MI355_SORT_T2"] or (16384 if entries >= 1 << 27 and fb <= 11 else 8192)
    p.update(t1=t1, t2=t2, tiles1=ceil_div(n, t1), l2_tiles_max=ceil_div(entries, t2) + p["regions"] + 8)
    # the reduction tail
    nb, chunk = 1 << kb, 64
    while chunk > nb:
        chunk >>= 1
    while chunk > k["MI355_REDUCE_MIN_CHUNK"] and (nb // chunk) * sets < k["MI355_REDUCE_CHAINS"]:
        chunk >>= 1
    quad_sums = (nb // chunk) * sets <= k["MI355_TAIL_COOP_MAX"] and bool(k["MI355_TAIL_COOP_MASK"] & 2)
    p.update(chunk=chunk, chunks_per_set=nb // chunk, sums="quad" if quad_sums else "one lane",
             tree_quad_max=k["MI355_TAIL_COOP_MAX"] if k["MI355_TAIL_COOP_MASK"] & 4 else 0, quad_final=bool(k["MI355_TAIL_COOP_MAX"] and k["MI355_TAIL_COOP_MASK"] & 8))
    return p


def batch_leaves(n, M, tab_c=None, rec_bytes=RECORD_BYTES, **settings):
    """the batch sizes a batch of M runs as: halves (M // 2, M - M // 2) while the plan says it must split"""
    if M > 1 and plan(n, M, tab_c, rec_bytes, **settings)["must_split"]:
        h = M // 2
        return batch_leaves(n, h, tab_c, rec_bytes, **settings) + batch_leaves(n, M - h, tab_c, rec_bytes, **settings)
    return [M]


def pipeline_chunks(n, M=1, **settings):
    """msm_chunks slices once n reaches 2^chunk_min_log, fewer while a slice would be shorter than a quarter of that; single polynomials only"""
    k = dict(DEFAULTS, **settings)
    chunks, min_log = k["MI355_MSM_CHUNKS"], k["chunk_min_log"]
    if chunks <= 1 or M != 1 or n < 1 << min_log:
        return 1
    while chunks > 1 and n // chunks < (1 << min_log) >> 2:
        chunks -= 1
    return chunks


def host_slices(n, M=1, tab_c=None, rec_bytes=RECORD_BYTES, **settings):
    """the cuts of the host-pointer MSM: a first slice of n / 16, each further one 1.7 times the last, the rest in the final slice, cut at multiples of 1024 from 2^20
    points on; [0, n] for batches, short vectors, MI355_HOST_CHUNKS = 1, a refused shape or more than 8 GiB of bucket sets -> (cuts, the plan of the biggest slice or None)"""
    k = dict(DEFAULTS, **settings)
    cut = []
    if M == 1 and n >= 1 << k["MI355_HOST_SLICE_MIN_LOG"] and k["MI355_HOST_CHUNKS"] > 1:
        w, tot, rem, ws, first = 1.0, 0.0, 1.0, [], 1.0 / 16.0
        while rem > 1e-9 and len(ws) + 1 < k["MI355_HOST_CHUNKS"]:
            take = min(rem, first * w)
            ws.append(take); rem -= take; w *= 1.7; tot += take
        if tot < 1.0 - 1e-9:
            ws.append(1.0 - tot)
        cut, acc, align = [0], 0.0, ~1023 if n >= 1 << 20 else ~0
        for x in ws[:-1]:
            acc += x
            c = min(n, int(acc * float(n)) & align)
            if cut[-1] < c < n:
                cut.append(c)
        cut.append(n)
    if len(cut) > 2:
        shape = plan(max(b - a for a, b in zip(cut, cut[1:])), 1, tab_c, rec_bytes, **settings)
        if not shape["refusal"] and shape["buckets"] * (len(cut) - 1) * rec_bytes <= 8 << 30:
            return cut, shape
    return [0, n], None


def boundaries(lo, hi):
    """every n in (lo, hi] with choose_c(n) != choose_c(n - 1) (the choice is a step function of n: bisection between the steps)"""
    out, n = [], lo
    while choose_c(n) != choose_c(hi):
        a, b = n, hi
        while b - a > 1:
            m = (a + b) // 2
            if choose_c(m) == choose_c(n):
                a = m
            else:
                b = m
        out.append(b); n = b
    return out
