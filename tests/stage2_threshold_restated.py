"""numpy restatement of the stage-2 threshold kernels (k_s2thr_* of csrc/stage2.hip), written from their normative comment: the monotone
32-bit key and the 4 x 8-bit rank select; the plain definition they must equal (reference trainer/eval_save_cosplbl_prop.py:243-254,
oracle/port.py:431-436); and the synthetic cases both test files share."""
import numpy as np

F32 = np.float32
METHODS = ('median', 'min')


def keys(sim):
    """uint32 keys of float32 similarities, ascending as the floats: sim + 0.0 (one key for -0.0 and +0.0), negatives with all bits
    flipped, non-negatives with the sign bit set."""
    u = (np.asarray(sim, dtype=F32) + F32(0.0)).astype(F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_to_float(key):
    key = np.asarray(key, dtype=np.uint32)
    return np.where(key & np.uint32(0x80000000), key ^ np.uint32(0x80000000), ~key).astype(np.uint32).view(F32)


def rank_select(key, rank):
    """The key of rank ``rank`` (ascending, 0-based) among ``key``, digit by digit from the top: per round a 256-bin histogram of the
    next digit of the keys that share the prefix so far; the digit whose bin holds the rank is appended and the bins below it are
    taken off the rank."""
    key = np.asarray(key, dtype=np.uint32)
    prefix, rank = np.uint32(0), int(rank)
    for shift in (24, 16, 8, 0):
        match = np.ones(key.shape, dtype=bool) if shift == 24 else ((key ^ prefix) >> np.uint32(shift + 8)) == 0
        hist = np.bincount(((key[match] >> np.uint32(shift)) & np.uint32(255)).astype(np.int64), minlength=256)
        upto = np.cumsum(hist)
        digit = int(np.searchsorted(upto, rank, side='right'))
        assert digit < 256 and hist[digit] > 0
        rank -= int(upto[digit] - hist[digit])
        prefix = np.uint32(prefix | np.uint32(digit << shift))
    return prefix


def thresholds(nn, nn_sim, n_proto, method):
    """float32 [n_proto] as the kernels compute it."""
    nn, nn_sim = np.asarray(nn).reshape(-1), np.asarray(nn_sim, dtype=F32).reshape(-1)
    thr = np.ones(n_proto, dtype=F32)
    for k in range(n_proto):
        key = keys(nn_sim[nn == k])
        if key.size:
            thr[k] = key_to_float(key.min() if method == 'min' else rank_select(key, (key.size - 1) // 2))
    return thr


def thresholds_plain(nn, nn_sim, n_proto, method):
    """The definition: the smallest element / the element of rank (cnt - 1) // 2 in ascending order; 1.0 for an empty set."""
    nn, nn_sim = np.asarray(nn).reshape(-1), np.asarray(nn_sim, dtype=F32).reshape(-1)
    thr = np.ones(n_proto, dtype=F32)
    for k in range(n_proto):
        sel = nn_sim[nn == k]
        if sel.size:
            thr[k] = sel.min() if method == 'min' else np.sort(sel)[(sel.size - 1) // 2]
    return thr


# ------------------------------------------------------------------------------------------------
# the synthetic cases: (HW, n_proto) x value pattern
# ------------------------------------------------------------------------------------------------
SHAPES = ((50 * 77, 1), (50 * 77, 7), (50 * 77, 300), (64 * 96, 1), (64 * 96, 7), (64 * 96, 300))
PATTERNS = ('equal', 'low_byte', 'top_byte', 'signs', 'duplicates', 'uniform')
SMALL_COUNTS = (0, 1, 2, 3, 4, 255, 256, 257)


def assignment(rs, HW, n_proto):
    """int32 [HW]: about a third of the pixels -1.  n_proto 1: that prototype owns every other pixel.  Otherwise the first prototypes
    get exactly the counts of SMALL_COUNTS (as many as n_proto and the pixels allow), one further id stays without a pixel and the rest
    share what is left at random -- in runs of 1..40 pixels, as neighbouring pixels share their prototype."""
    nn = np.full(HW, -1, dtype=np.int32)
    free = rs.permutation(HW)[:HW - HW // 3]
    if n_proto == 1:
        nn[free] = 0
        return nn
    fixed = SMALL_COUNTS[:n_proto - 2]
    at = 0
    for k, c in enumerate(fixed):
        nn[free[at:at + c]] = k
        at += c
    rest = np.sort(free[at:])
    others = np.arange(len(fixed), n_proto - 1)                   # id n_proto - 1 is carried by no pixel
    i = 0
    while i < rest.size:
        run = int(rs.randint(1, 41))
        nn[rest[i:i + run]] = rs.choice(others)
        i += run
    return nn


def values(rs, pattern, nn, n_proto):
    """float32 [HW] similarities for one value pattern."""
    HW = nn.size
    if pattern == 'equal':                        # every round has one bin
        return np.full(HW, F32(0.8125))
    if pattern == 'low_byte':                     # the last round decides
        return (np.uint32(0x3f400000) | rs.randint(0, 256, HW).astype(np.uint32)).view(F32)
    if pattern == 'top_byte':                     # only the top byte differs (signs and exponents far apart; finite)
        top = rs.choice(np.array([0x00, 0x01, 0x3e, 0x3f, 0x40, 0x7e, 0x80, 0x81, 0xbe, 0xbf, 0xc0, 0xfe], dtype=np.uint32), HW)
        return ((top << np.uint32(24)) | np.uint32(0x00345678)).view(F32)
    if pattern == 'signs':                        # negative and positive values, both zeros
        v = rs.choice(np.array([-0.75, -0.5, -1e-3, -0.0, 0.0, 1e-3, 0.5, 0.75], dtype=F32), HW)
        v[rs.rand(HW) < 0.5] *= F32(0.5)
        return v.astype(F32)
    if pattern == 'duplicates':                   # per prototype at most three distinct values: equal values straddle the median rank
        base = rs.uniform(-1, 1, (n_proto, 3)).astype(F32)
        return base[np.maximum(nn, 0), rs.randint(0, 3, HW)]
    assert pattern == 'uniform'
    return rs.uniform(-1, 1, HW).astype(F32)


def case(HW, n_proto, pattern):
    """(nn int32 [HW], nn_sim float32 [HW]) of one case; the same arrays on every call."""
    rs = np.random.RandomState(1000 * PATTERNS.index(pattern) + HW % 997 + n_proto)
    nn = assignment(rs, HW, n_proto)
    return nn, np.ascontiguousarray(values(rs, pattern, nn, n_proto), dtype=F32)


CASES = [(HW, n, p) for HW, n in SHAPES for p in PATTERNS]
