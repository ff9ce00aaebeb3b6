"""numpy restatement of the tracer-particle scheme (iamr_amd/csrc/k_particles.hip): the yardstick of tests/test_cpu_particles.py and
tests/test_gpu_particles.py.

The scheme is TracerParticleContainer::AdvectWithUmac / ParticleContainer::Redistribute of AMReX as recalled from upstream; AMReX is not in
the reference tree, so none of this is pinned against it.  The two counts follow NavierStokesBase::ParticleDerive
(Source/NavierStokesBase.cpp:3996-4048), which is.

Conventions: a level is dict(n (cells, 3), dlo (domain low index, 3), dx (3), boxes [(lo, hi), ...] in the level's index space); the domain
is prob_lo, prob_hi, periodic (3 each).  A face array of component d is a numpy array over an index box with origin `lo` (face-centred in d,
cell-centred in the other two directions), ghost faces included.
"""
import numpy as np


# ---- MAC interpolation and the two passes ---------------------------------------------------------------------------------------------------
def interp_face(F, flo, d, x, prob_lo, dx, dlo, dhi, periodic):
    """trilinear interpolation of the face array F (origin flo) of component d at the positions x (n, 3).  l_e = (x_e - prob_lo_e) / dx_e -
    (e == d ? 0 : 1/2), i_e = floor(l_e), weights l_e - i_e and its complement.  At non-periodic domain faces the stencil indices are
    clamped to the faces / cells of the domain (dlo .. dhi cells); everywhere to the array."""
    x = np.asarray(x, dtype=np.float64)
    i0, i1, w = [], [], []
    for e in range(3):
        l = (x[:, e] - prob_lo[e]) / dx[e] - (0.0 if e == d else 0.5)
        fl = np.floor(l)
        w.append(l - fl)
        a = fl.astype(np.int64) + dlo[e]
        b = a + 1
        if not periodic[e]:
            lo, hi = dlo[e], dhi[e] + (1 if e == d else 0)
            a, b = np.clip(a, lo, hi), np.clip(b, lo, hi)
        a, b = np.clip(a, flo[e], flo[e] + F.shape[e] - 1), np.clip(b, flo[e], flo[e] + F.shape[e] - 1)
        i0.append(a - flo[e])
        i1.append(b - flo[e])
    wx, wy, wz = w
    f = lambda a, b, c: F[a, b, c]
    # a + w (b - a) in x, then y, then z: a uniform field is reproduced to the bit
    lerp = lambda a, b, t: a + t * (b - a)
    a00, a10 = lerp(f(i0[0], i0[1], i0[2]), f(i1[0], i0[1], i0[2]), wx), lerp(f(i0[0], i1[1], i0[2]), f(i1[0], i1[1], i0[2]), wx)
    a01, a11 = lerp(f(i0[0], i0[1], i1[2]), f(i1[0], i0[1], i1[2]), wx), lerp(f(i0[0], i1[1], i1[2]), f(i1[0], i1[1], i1[2]), wx)
    return lerp(lerp(a00, a10, wy), lerp(a01, a11, wy), wz)


def advect(x, ids, umac, umac_lo, dt, prob_lo, dx, dlo, dhi, periodic, fixed_dir=-1):
    """the two passes for particles that read ONE set of face arrays umac[d] (origins umac_lo[d]): pass 1  r = x, x += dt/2 v(x);
    pass 2  x = r + dt v(x), r = v.  A particle with id <= 0 is skipped.  Nothing is wrapped between the passes.  -> (x_new, r_new)"""
    x = np.array(x, dtype=np.float64)
    live = np.asarray(ids) > 0

    def vel(pos):
        v = np.stack([interp_face(umac[d], umac_lo[d], d, pos, prob_lo, dx, dlo, dhi, periodic) for d in range(3)], axis=1)
        if fixed_dir >= 0:
            v[:, fixed_dir] = 0.0
        return v

    r = x.copy()
    xh = x + (0.5 * dt) * vel(x)
    v = vel(xh)
    xn = r + dt * v
    return np.where(live[:, None], xn, x), np.where(live[:, None], v, 0.0), live


# ---- redistribution -----------------------------------------------------------------------------------------------------------------------
def wrap(x, lo, hi):
    L = hi - lo
    x = x - L * np.floor((x - lo) / L)
    x = np.where(x >= hi, lo, x)
    return np.where(x < lo, lo, x)


def cell_of(level, x, prob_lo):
    """cell (relative to the domain's low corner) of the positions x, inside the domain"""
    c = np.empty(x.shape, dtype=np.int64)
    for e in range(3):
        l = np.floor((x[:, e] - prob_lo[e]) / level["dx"][e])
        c[:, e] = np.clip(l, 0.0, level["n"][e] - 1).astype(np.int64)
    return c


def box_holding(level, c, grow=0, shift=(0, 0, 0)):
    """lowest index of a box of the level whose region grown by `grow` holds the cell c (relative to the domain low corner) shifted by
    `shift` domain lengths, or -1"""
    for b, (lo, hi) in enumerate(level["boxes"]):
        if all(lo[e] - grow <= c[e] + shift[e] * level["n"][e] + level["dlo"][e] <= hi[e] + grow for e in range(3)):
            return b
    return -1


def redistribute(x, ids, lev, box, levels, prob_lo, prob_hi, periodic, lev_min, lev_max, ngrow):
    """-> (x, level, box, status) per particle; status 0 kept, 1 removed beyond a non-periodic face, 2 cannot be placed, 3 invalid (id <= 0).
    Particles of the levels below lev_min are left alone.  Rule: wrap periodic coordinates; the finest level <= lev_max whose valid boxes
    hold the particle's cell; failing that and with ngrow > 0 the box of lev_min with the lowest index whose ngrow-grown region holds the
    cell or a periodic image of it (of several images the one shifted in the fewest directions, the cell itself first) -- the particle
    then takes that image's position x + s (prob_hi - prob_lo)."""
    x = np.array(x, dtype=np.float64)
    n = x.shape[0]
    lev, box = np.array(lev, dtype=np.int64), np.array(box, dtype=np.int64)
    status = np.zeros(n, dtype=np.int64)
    lev_max = min(lev_max, len(levels) - 1)
    for p in range(n):
        if ids[p] <= 0:
            status[p] = 3
            continue
        if lev[p] < lev_min:
            continue
        for e in range(3):
            if periodic[e]:
                x[p, e] = wrap(x[p, e], prob_lo[e], prob_hi[e])
        if not all(prob_lo[e] <= x[p, e] < prob_hi[e] for e in range(3)):
            status[p] = 1
            continue
        found = False
        for L in range(lev_max, lev_min - 1, -1):
            c = cell_of(levels[L], x[p:p + 1], prob_lo)[0]
            b = box_holding(levels[L], c)
            if b >= 0:
                lev[p], box[p], found = L, b, True
                break
        if not found and ngrow > 0:
            L = levels[lev_min]
            c = cell_of(L, x[p:p + 1], prob_lo)[0]
            best = None
            for s2 in (-1, 0, 1):
                for s1 in (-1, 0, 1):
                    for s0 in (-1, 0, 1):
                        s = (s0, s1, s2)
                        if any(s[e] != 0 and not periodic[e] for e in range(3)):
                            continue
                        b = box_holding(L, c, ngrow, s)
                        ns = sum(1 for v in s if v != 0)
                        if b >= 0 and (best is None or (b, ns) < (best[0], best[2])):
                            best = (b, s, ns)
            if best is not None:
                lev[p], box[p], found = lev_min, best[0], True
                for e in range(3):
                    if best[1][e] != 0:
                        x[p, e] = x[p, e] + float(best[1][e]) * (prob_hi[e] - prob_lo[e])
        if not found:
            status[p] = 2
    return x, lev, box, status


# ---- counts -----------------------------------------------------------------------------------------------------------------------------
def particle_count(x, lev, box, levels, prob_lo, l):
    """array over the domain of level l: the number of level-l particles in every VALID cell of their own box"""
    out = np.zeros(tuple(levels[l]["n"]))
    L = levels[l]
    for p in np.nonzero(np.asarray(lev) == l)[0]:
        c = [int(np.floor((x[p, e] - prob_lo[e]) / L["dx"][e])) for e in range(3)]
        lo, hi = L["boxes"][box[p]]
        if all(0 <= c[e] < L["n"][e] and lo[e] <= c[e] + L["dlo"][e] <= hi[e] for e in range(3)):
            out[tuple(c)] += 1.0
    return out


def total_particle_count(x, lev, box, levels, prob_lo, l):
    """particle_count of level l plus the counts of every finer level coarsened onto l (NavierStokesBase.cpp:4005-4048: fine cells with a
    positive count are added to their coarse cell; only where level l has a box)"""
    out = particle_count(x, lev, box, levels, prob_lo, l)
    covered = np.zeros(out.shape, dtype=bool)
    for lo, hi in levels[l]["boxes"]:
        covered[tuple(slice(lo[e] - levels[l]["dlo"][e], hi[e] - levels[l]["dlo"][e] + 1) for e in range(3))] = True
    for lf in range(l + 1, len(levels)):
        fine = particle_count(x, lev, box, levels, prob_lo, lf)
        trr = [levels[lf]["n"][e] // levels[l]["n"][e] for e in range(3)]
        for c in zip(*np.nonzero(fine > 0)):
            cc = tuple(c[e] // trr[e] for e in range(3))
            if covered[cc]:
                out[cc] += fine[c]
    return out
