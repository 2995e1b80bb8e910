"""Random / adversarial seed generators for the tests (numpy only; deterministic by seed)."""
import numpy as np


def mutate(rng, ref, n, sub, indel):
    """Derive an n-base read from reference bases `ref` with substitutions and indels."""
    out = []
    rp = 0
    while len(out) < n:
        r = rng.random()
        if r < indel / 2:
            out.append(int(rng.integers(0, 4)))
        elif r < indel:
            rp += int(rng.integers(1, 12))
        else:
            b = int(ref[rp]) if rp < len(ref) else int(rng.integers(0, 4))
            rp += 1
            if rng.random() < sub:
                b = (b + 1 + int(rng.integers(0, 3))) & 3
            out.append(b)
    return np.array(out, dtype=np.uint8)


def general_matrix(rng, off_hi=9):
    """A 5x5 scoring matrix mat[target][query] that no symmetry protects: entries in [-9, 9], the four base diagonals in 1..9,
    the other base entries in [-9, off_hi], the N row and the N column drawn independently of each other.  Redrawn until it
    differs from its transpose among the bases and on the N row / column, and from its image under complementing both codes
    and under complementing either one: a kernel that swaps the indices, or complements the wrong one, reads another matrix."""
    comp = [3, 2, 1, 0, 4]
    while True:
        m = rng.integers(-9, off_hi + 1, (5, 5)).astype(np.int8)
        for k in range(4):
            m[k, k] = rng.integers(1, 10)
        m[4, :] = rng.integers(-9, 10, 5)
        m[:4, 4] = rng.integers(-9, 10, 4)
        both = m[comp][:, comp]
        if ((m[:4, :4] != m[:4, :4].T).sum() >= 6 and (m[4, :4] != m[:4, 4]).sum() >= 2 and (m != both).sum() >= 6 and
                (m != m[comp]).sum() >= 6 and (m != m[:, comp]).sum() >= 6 and (m != both.T).sum() >= 6):
            return m


GLOBAL_PENS = [(5, 2, 7, 1), (11, 3, 4, 2), (0, 2, 1, 1), (3, 1, 9, 4)]   # (o_del, e_del, o_ins, e_ins): insertion != deletion in both


def global_pair(rng, ql, lmax=None, drift=6, sub=0.08, indel=0.10, nrate=0.03, junk=0.2):
    """A (query, target) pair for ksw_global2 whose narrow bands bind: a query of ql codes 0..4 read with many indels off a target
    of ql +- drift bases (mutate's skips of 1..11 bases move the path off the diagonal), or with probability `junk` unrelated
    to it; with lmax the junk target has any length 0..lmax, so |qlen - tlen| is large too.  N (code 4) at rate nrate in both."""
    if rng.random() < junk:
        tl = int(rng.integers(0, lmax + 1)) if lmax is not None else max(0, ql + int(rng.integers(-drift, drift + 1)))
        t = rng.integers(0, 4, tl).astype(np.uint8)
        q = rng.integers(0, 4, ql).astype(np.uint8)
    else:
        tl = max(0, ql + int(rng.integers(-drift, drift + 1)))
        if lmax is not None:
            tl = min(tl, lmax)
        t = rng.integers(0, 4, tl).astype(np.uint8)
        q = mutate(rng, t, ql, sub, indel)
    q[rng.random(ql) < nrate] = 4
    t[rng.random(tl) < nrate] = 4
    return q, t


def extremes_matrix(rng):
    """The matrix of test_gpu_global_long.test_general_matrix_extremes_and_ns: entries from {-128, -127, -1, 0, 1, 126, 127},
    the diagonal 126 / 127, N against N -128."""
    mat = rng.choice(np.array([-128, -127, -1, 0, 1, 126, 127], dtype=np.int8), 25)
    for k in range(5):
        mat[k * 5 + k] = 127 if k % 2 else 126
    mat[4 * 5 + 4] = -128
    return mat


def limit_matrix():
    """a = 127 on the four base diagonals, -128 everywhere else (N against N too): the value limits of an int8 matrix"""
    mat = np.full((5, 5), -128, dtype=np.int8)
    for k in range(4):
        mat[k, k] = 127
    return mat.ravel()


def clean_gap_pair(rng, n, gap, deletion, at=None):
    """n bases of codes 0..2 against themselves with one block of `gap` bases of code 3 put into the target (deletion) or into
    the query: the block is the only place the extra bases can go without losing a match.  Returns (query, target)."""
    s = rng.integers(0, 3, n).astype(np.uint8)
    at = n // 2 if at is None else at
    long = np.concatenate([s[:at], np.full(gap, 3, np.uint8), s[at:]])
    return (s, long) if deletion else (long, s)


def clean_gap_cigar(n, gap, deletion, at=None):
    """the one alignment of clean_gap_pair that keeps every match: [(op, len), ...] with 0 = M, 1 = I, 2 = D"""
    at = n // 2 if at is None else at
    return [(op, ln) for op, ln in ((0, at), (2 if deletion else 1, gap), (0, n - at)) if ln]


def random_seeds(rng, n, qmin=1, qmax=140, tfac=2.0, sub=0.03, indel=0.01, junk=0.2, nrate=0.0, h0max=60,
                 both_sides=True, tmin=0):
    """List of seed dicts for host.make_tasks()."""
    seeds = []
    for k in range(n):
        s = {"h0": int(rng.integers(1, h0max + 1))}
        for side in ("l", "r"):
            if side == "l" and (not both_sides or rng.random() < 0.2):
                continue
            if side == "r" and both_sides and rng.random() < 0.1 and "lq" in s:
                continue
            ql = int(rng.integers(qmin, qmax + 1))
            tl = max(tmin, int(rng.integers(0, int(ql * tfac) + 2)))
            t = rng.integers(0, 4, tl).astype(np.uint8)
            if rng.random() < junk:
                q = rng.integers(0, 4, ql).astype(np.uint8)
            else:
                q = mutate(rng, t, ql, sub, indel)
            if nrate > 0:
                q[rng.random(ql) < nrate] = 4
                t[rng.random(tl) < nrate] = 4
            s[side + "q"], s[side + "t"] = q, t
        s["init_score"] = -1 if rng.random() < 0.8 else int(rng.integers(-1, 50))
        s["tag"] = int(rng.integers(0, 2 ** 32))
        seeds.append(s)
    return seeds


def query_has_n(tasks, arena, side):
    """Per task: does the left (side 0) / right (side 1) query hold a base code >= 4?  (the binning's second key)"""
    import numpy as np
    pf, lf = ("lquery", "lqlen") if side == 0 else ("rquery", "rqlen")
    base = arena.ctypes.data
    a = np.asarray(arena).view(np.uint8).ravel()
    out = np.zeros(len(tasks), bool)
    for i, (p, l) in enumerate(zip(tasks[pf], tasks[lf])):
        if l:
            o = int(p) - base
            out[i] = bool((a[o:o + int(l)] >= 4).any())
    return out
