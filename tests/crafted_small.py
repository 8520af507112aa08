"""Camera systems and batches built to order for the direct tests of the dense small-system path (csrc/lsfm_small.hip, k_small_solve;
test_crafted_small_cpu.py, test_gpu_small_crafted.py): plain numpy, no GPU, nothing of the reference.  The systems are
crafted_system.craft()'s -- positive semi-definite by construction, a prior on U, +-1 decade of scaling, repeats cut element by
element.  Which code of k_small_solve runs hangs on the index arrays, the pose count and the layout of the batch alone; describe()
restates the kernel's walk over them -- chunks of run pointers, super-passes, passes, the W rows parked in LDS, the strip masks -- so
that test_crafted_small_cpu.py can assert that a case reaches the branch it is named for."""
import functools

import numpy as np

import crafted_system as cs
from common import dense_reference_solve
from refdump import dense_info

# lsfm_small.hip (test_crafted_small_cpu.py reads them from the source)
SM_PASS, SM_SUPER, SM_CHUNK, SM_WROWS = 16, 64, 256, 1024
STRIPS = ((2, 1), (5, 2), (8, 3), (16, 6))  # small_solve_strips: poses up to -> 16-row strips of the instance
PARKED = SM_WROWS // 6                      # 170: the blocks of a super-pass that lie in LDS with all six rows
DECADES = 1


def _split(n, poses, run, last=None, **kw):
    """n features as craft()'s tiles of 128, all seen by `poses` with runs of `run`; last: (poses, run) of a short last tile that has
    too few features to be seen by all of them"""
    out = [dict(poses=np.asarray(poses), run=run, **kw) for _ in range(n // cs.TILE)]
    if n % cs.TILE:
        lp, lr = last if last is not None else (poses, run)
        out.append(dict(n=n % cs.TILE, poses=np.asarray(lp), run=lr, **kw))
    return out


_A = np.arange
# name -> (m, tiles, keyword arguments of craft)
CASES = {
    "p1": (1, _split(17, [0], (1, 1)), {}),
    "p2a": (2, _split(16, _A(2), (1, 2)), {}),
    "p2b": (2, _split(257, _A(2), (1, 2), last=([1], (1, 1))), {"offdiag": True}),
    "p3": (3, _split(65, _A(3), (1, 3)), {"offdiag": True}),
    "p5a": (5, _split(64, _A(5), (1, 3)), {}),
    "p5b": (5, _split(321, _A(5), (1, 4)), {"offdiag": True}),
    "p6": (6, _split(15, _A(6), (1, 4)), {}),
    "p8a": (8, _split(256, _A(8), (1, 3)), {}),
    "p8b": (8, _split(513, _A(8), (2, 8), last=([3, 6], (2, 2))), {"offdiag": True}),
    "p9": (9, _split(63, _A(9), (1, 4)), {"offdiag": True}),
    "p16a": (16, _split(1, _A(16), (16, 16)), {}),
    # tiles seen by a few poses each: passes that touch two to four of the six strips.  The six rows of poses 2, 5, 10 and 13 lie in two
    # strips: in the tiles seen by (5, 10) and by (2, 13) the second strip of each is on through that pose alone.  A ragged last tile
    # that all poses see
    "p16b": (16, [dict(poses=_A(0, 4), run=(1, 3)), dict(poses=np.array([5, 10]), run=(1, 2)), dict(poses=_A(10, 16), run=(1, 3)),
                  dict(poses=np.array([2, 13]), run=(1, 2)), dict(n=88, poses=_A(16), run=(1, 3))], {"offdiag": True}),
    "p16c": (16, _split(192, _A(16), (16, 16)), {}),
    "w170": (8, _split(34, _A(8), (5, 5)), {"dup": 0.0}),
    "w171": (8, _split(57, _A(8), (3, 3)), {"dup": 0.0}),
    "u16": (16, _split(200, np.r_[_A(0, 8), _A(11, 16)], (1, 3)), {"offdiag": True}),
    "du5": (5, _split(100, _A(5), (1, 3)), {"offdiag": True, "split_u": True}),
    "g3": (3, _split(80, _A(3), (1, 3)), {"offdiag": True}),
    "g9": (9, _split(150, _A(9), (2, 5)), {"offdiag": True}),
    "v8": (8, _split(100, _A(8), (1, 3)), {"bad_v": (50, 1e-3)}),
}
MONO = ("g3", "g9")
GOOD = [k for k in CASES if k != "v8"]
MIXED = ("p2a", "p16b", "p1", "p5b", "p9", "p3", "w171", "p6")  # one launch: the 6-strip instance for all
MANY = ("p1", "p2a", "p3", "p6")                                # the systems the 2048-segment batch cycles over


@functools.lru_cache(maxsize=None)
def system(name):
    m, tiles, kw = CASES[name]
    return cs.craft(m, tiles, 50000 + sorted(CASES).index(name), decades=DECADES, **kw)


def rhs_of(J, seed):
    """crafted_system.rhs's right-hand sides: ea with the scalars' scales, eb a unit normal"""
    rng = np.random.default_rng(seed)
    ea = np.sqrt(np.diag(cs.dense_u(J))) * rng.standard_normal(6 * J["m"])
    return ea, rng.standard_normal(3 * J["n"])


@functools.lru_cache(maxsize=None)
def rhs(name):
    return rhs_of(system(name), 77 + sorted(CASES).index(name))


def gauge(J):
    """crafted_system.gauge for systems of as few as three poses: the block of one pose that features see and one scalar of another
    (Ref, ScaP, Fix, Sign, FixBlk)"""
    seen = np.unique(J["photo"])
    ref, other = int(seen[min(2, len(seen) - 2)]), int(seen[min(7, len(seen) - 1)])
    return [ref, 6 * ref, 6 * other + 4, -1, other]


def gauge_mask(J, sa):
    fx = np.zeros(6 * J["m"], bool)
    fx[6 * sa[0]:6 * sa[0] + 6] = True
    fx[sa[2]] = True
    return fx


@functools.lru_cache(maxsize=None)
def expected_x(name):
    """(expected state, mono, sa): common.dense_reference_solve on the full normal equations.  Shared, never changed."""
    J = system(name)
    ea, eb = rhs(name)
    mono = name in MONO
    sa = gauge(J) if mono else None
    x = dense_reference_solve(J, ea, eb, mono, sa)
    x.setflags(write=False)
    return x, mono, sa


def solve_many(J, EA, EB):
    """dense_reference_solve's method -- LU of the full normal equations, residuals in long double until the correction is below 1e-17
    relative -- for k right-hand sides at once (EA [k, 6 m], EB [k, 3 n]); returns [k, 6 m + 3 n]"""
    import scipy.linalg as sl
    A = dense_info(J)
    A = np.triu(A) + np.triu(A, 1).T
    b = np.concatenate([np.asarray(EA, np.float64), np.asarray(EB, np.float64)], axis=1).T
    Al, bl = A.astype(np.longdouble), b.astype(np.longdouble)
    lu = sl.lu_factor(A)
    x = sl.lu_solve(lu, b)
    xl = x.astype(np.longdouble)
    for _ in range(8):
        dx = sl.lu_solve(lu, np.asarray(bl - Al @ xl, np.float64))
        xl = xl + dx.astype(np.longdouble)
        if np.all(np.max(np.abs(dx), axis=0) <= 1e-17 * np.max(np.abs(x), axis=0)):
            break
    return np.asarray(xl, np.float64).T


def without_features(J):
    """the poses of a system alone: U x = ea"""
    return dict(J, n=0, W=np.zeros((0, 18)), V=np.zeros((0, 9)), photo=np.zeros(0, np.int32), feature=np.zeros(0, np.int32))


def batch(parts):
    """[(J, ea, eb)] back to back in one numbering, as a tree level lays its joins out: pose_off / feat_off / u_off [G + 1], the index
    arrays shifted by the first pose / feature of their system"""
    po = np.cumsum([0] + [int(J["m"]) for J, _, _ in parts])
    fo = np.cumsum([0] + [int(J["n"]) for J, _, _ in parts])
    uo = np.cumsum([0] + [len(J["Ui"]) for J, _, _ in parts])
    cat = lambda k, dt, shift=None: np.concatenate([(np.asarray(J[k]).reshape(-1) + (0 if shift is None else shift[g])).astype(dt) for g, (J, _, _) in enumerate(parts)])
    return dict(pose_off=po.astype(np.int32), feat_off=fo.astype(np.int32), u_off=uo.astype(np.int32),
                U=cat("U", np.float64), Ui=cat("Ui", np.int32, po), Uj=cat("Uj", np.int32, po),
                W=cat("W", np.float64), photo=cat("photo", np.int32, po), feature=cat("feature", np.int32, fo), V=cat("V", np.float64),
                ea=np.concatenate([np.asarray(ea, np.float64) for _, ea, _ in parts]), eb=np.concatenate([np.asarray(eb, np.float64) for _, _, eb in parts]))


def named_batch(names):
    return batch([(system(k),) + rhs(k) for k in names])


def segment(B, g, xp, xf):
    """the state of system g of a batch in a single system's layout"""
    return np.concatenate([xp[6 * B["pose_off"][g]:6 * B["pose_off"][g + 1]], xf[3 * B["feat_off"][g]:3 * B["feat_off"][g + 1]]])


# ---- the kernel's walk over the index arrays ----------------------------------------------------------------------------------------------
STRADDLE = [p for p in range(16) if (6 * p) >> 4 != (6 * p + 5) >> 4]  # poses whose six rows lie in two 16-row strips


def strips_of(m):
    return next(s for cap, s in STRIPS if m <= cap)


def describe(J, strips=None):
    """What k_small_solve meets on the index arrays of one system, at the instance of `strips` strips (default: its own):
    instance; loads (first feature of every run-pointer chunk loaded: the buffers alternate) and last_entry (the highest entry of a
    chunk that is read); supers: per super-pass dict(feats, blocks, rep_in, rep_behind -- repeated (pose, feature) blocks whose second
    block lies inside / behind the rows parked in LDS); passes: per pass dict(feats, mask, off -- tiles of the instance that the
    mask switches off); tiles (of the instance); unseen (poses without a block)."""
    m, n = int(J["m"]), int(J["n"])
    ntr = strips_of(m) if strips is None else strips
    ph, fe = np.asarray(J["photo"], np.int64), np.asarray(J["feature"], np.int64)
    fptr = np.searchsorted(fe, np.arange(n + 1))
    tiles = [(i, j) for j in range(ntr) for i in range(j + 1)]
    loads, c0, last_entry, supers, passes = [], 0, 0, [], []
    for s0 in range(0, n, SM_SUPER):
        if s0 == 0 or s0 - c0 >= SM_CHUNK:  # (prefetch's rule)
            c0 = s0
            loads.append(s0)
        nfs = min(SM_SUPER, n - s0)
        last_entry = max(last_entry, s0 - c0 + nfs)
        qbs = fptr[s0]
        rep_in = rep_behind = 0
        for f in range(s0, s0 + nfs):
            run = ph[fptr[f]:fptr[f + 1]]
            for k in range(1, len(run)):
                if run[k] in run[:k]:
                    e = fptr[f] + k - qbs
                    if 6 * e + 5 < SM_WROWS:
                        rep_in += 1
                    else:
                        rep_behind += 1
        supers.append(dict(feats=nfs, blocks=int(fptr[s0 + nfs] - qbs), rep_in=rep_in, rep_behind=rep_behind))
        for q0 in range(s0, s0 + nfs, SM_PASS):
            nf = min(SM_PASS, n - q0)
            mask = 0
            for p in np.unique(ph[fptr[q0]:fptr[q0 + nf]]):
                mask |= (1 << ((6 * p) >> 4)) | (1 << ((6 * p + 5) >> 4))
            passes.append(dict(feats=nf, mask=mask, off=sum(1 for i, j in tiles if not ((mask >> i) & (mask >> j) & 1))))
    return dict(instance=strips_of(m), loads=loads, last_entry=last_entry, supers=supers, passes=passes, tiles=len(tiles),
                unseen=np.setdiff1d(np.arange(m), np.unique(ph)).tolist(), runs=np.diff(fptr))
