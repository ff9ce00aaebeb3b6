"""Plain reference of the viscous tensor operator (the MLTensorOp role: iamr_amd/csrc/k_tensor.hip, mlmg.hip) for the test-suite, and
the inputs its CPU and GPU tests share.

Written from the operator's definition on ONE global array in np.longdouble, vectorised with slices; no device code and no oracle code
in it (tests/test_cpu_tensor_ref.py compares it with oracle/orc_tensor.c, tests/test_gpu_tensor_bc_matrix.py the kernels with it).

Arrays: velocity (nx + 2, ny + 2, nz + 2, 3) with one ghost layer, array index = cell index + 1; face arrays of direction d have
n_d + 1 entries along d (face f lies between the cells f - 1 and f) and no ghost cells.

    y = a acoef u - b div(tau),     tau = eta (grad u + grad u^T) - 2/3 eta (div u) I,

tau_nd on a d-face: the normal derivative is the difference of the two cells of the face, a transverse derivative the mean of the
central differences at those two cells."""
import functools
import itertools
import numpy as np

LD = np.longdouble
PER, DIR, NEU, ODD = 0, 101, 102, 104          # LinOpBCType codes: interior / periodic, Dirichlet, Neumann, reflect_odd


# ---------------------------------------------------------------------------------------------------------------------------
# the boundary step
def lagrange_weights(NX):
    """weights at -1/2 of the polynomial through the boundary value at 0 and the cell centres 1/2, 3/2, ... (NX points)"""
    x = [LD(0), LD(1) / 2, LD(3) / 2, LD(5) / 2][:NX]
    xi = -LD(1) / 2
    c = []
    for j in range(NX):
        w = LD(1)
        for i in range(NX):
            if i != j:
                w = w * (xi - x[i]) / (x[j] - x[i])
        c.append(w)
    return c


def _ix(fixed):
    """index tuple of the velocity array (without the component): `fixed` direction -> index, the interior everywhere else"""
    return tuple(fixed.get(d, slice(1, -1)) for d in range(3))


def _rule(out, bcval, n, d, side, bct, fixed, NX, inhomog):
    """the one-dimensional rule of the face (d, side) along d for component n, on the cells `fixed` (transverse directions) selects:
    the value of the ghost cell from the cells behind it as they are in `out`"""
    nd = out.shape[d] - 2
    g, s = (0, 1) if side == 0 else (nd + 1, -1)

    def at(m):
        f = dict(fixed); f[d] = g + m * s
        return out[_ix(f) + (n,)]
    if bct == NEU:
        return at(1)
    if bct == ODD:
        return -at(1)
    assert bct == DIR, bct
    c = lagrange_weights(NX)
    f = dict(fixed); f[d] = g
    v = c[0] * (bcval[_ix(f) + (n,)] if inhomog else LD(0))
    for m in range(1, NX):
        v = v + c[m] * at(m)
    return v


def fill_ghosts(u, bcval, per, lobc9, hibc9, maxorder, inhomog=True):
    """the ghost layer of the operator: faces, then edges, then corners outside non-periodic faces -- each the mean, over its
    non-periodic exterior directions, of the face rule applied along that direction to the cells already filled (Dirichlet 101:
    Lagrange extrapolation through the boundary value stored in that ghost cell of bcval, NX = min(n_d + 1, maxorder) points; Neumann
    102: the first cell behind; reflect_odd 104: minus that cell); periodic directions are images.  lobc9 / hibc9: [3 n + d], one
    triple per component.  Returns a new longdouble array; the valid cells of u are kept."""
    out = np.array(u, dtype=LD)
    bv = np.array(bcval, dtype=LD)
    n = [out.shape[d] - 2 for d in range(3)]
    walls = [d for d in range(3) if not per[d]]
    NX = [min(n[d] + 1, maxorder) for d in range(3)]
    bc = lambda c, d, side: (lobc9 if side == 0 else hibc9)[3 * c + d]
    gidx = lambda d, side: 0 if side == 0 else n[d] + 1
    for nout in (1, 2, 3):
        for dirs in itertools.combinations(walls, nout):
            for sides in itertools.product((0, 1), repeat=nout):
                fixed = {d: gidx(d, s) for d, s in zip(dirs, sides)}
                for c in range(3):
                    acc = LD(0)
                    for d, s in zip(dirs, sides):
                        rest = {e: v for e, v in fixed.items() if e != d}
                        acc = acc + _rule(out, bv, c, d, s, bc(c, d, s), rest, NX[d], inhomog)
                    out[_ix(fixed) + (c,)] = acc / LD(nout)
    for d in range(3):
        if per[d]:
            lo = [slice(None)] * 3; hi = [slice(None)] * 3; src_lo = [slice(None)] * 3; src_hi = [slice(None)] * 3
            lo[d], src_lo[d], hi[d], src_hi[d] = 0, n[d], n[d] + 1, 1
            out[tuple(lo)] = out[tuple(src_lo)]
            out[tuple(hi)] = out[tuple(src_hi)]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the operator
def _fv(A, d, side, t=None, off=0):
    """A (cells with one ghost layer) seen from the d-faces: the cell below (side 0) / above (1) every face, moved by `off` along t"""
    s = [slice(1, -1)] * 3
    nd = A.shape[d] - 2
    s[d] = slice(0, nd + 1) if side == 0 else slice(1, nd + 2)
    if t is not None:
        nt = A.shape[t] - 2
        s[t] = slice(1 + off, 1 + off + nt)
    return A[tuple(s)]


def stress(u, eta, h):
    """tau[d][..., n] = tau_nd on the d-faces"""
    u = np.asarray(u, dtype=LD)
    h = [LD(v) for v in h]
    tau = []
    for d in range(3):
        e = np.asarray(eta[d], dtype=LD)
        e = e[..., 0] if e.ndim == 4 else e
        dn = lambda c: (_fv(u[..., c], d, 1) - _fv(u[..., c], d, 0)) / h[d]
        dt = lambda c, t: ((_fv(u[..., c], d, 1, t, 1) - _fv(u[..., c], d, 1, t, -1))
                           + (_fv(u[..., c], d, 0, t, 1) - _fv(u[..., c], d, 0, t, -1))) / (4 * h[t])
        T = np.empty(e.shape + (3,), dtype=LD)
        for c in range(3):
            if c == d:
                T[..., c] = e * (LD(4) / 3 * dn(d) - LD(2) / 3 * sum(dt(t, t) for t in range(3) if t != d))
            else:
                T[..., c] = e * (dn(c) + dt(d, c))
        tau.append(T)
    return tau


def apply(u_filled, eta, a, b, acoef, h):
    """y = a acoef u - b div(tau) on the valid cells; acoef None: no a-term"""
    tau = stress(u_filled, eta, h)
    n = [u_filled.shape[d] - 2 for d in range(3)]
    y = np.zeros(tuple(n) + (3,), dtype=LD)
    for d in range(3):
        hi = [slice(None)] * 3; lo = [slice(None)] * 3
        hi[d], lo[d] = slice(1, n[d] + 1), slice(0, n[d])
        y -= LD(b) * (tau[d][tuple(hi)] - tau[d][tuple(lo)]) / LD(h[d])
    if acoef is not None and a != 0:
        ac = np.asarray(acoef, dtype=LD)
        ac = ac[..., 0] if ac.ndim == 4 else ac
        y += LD(a) * ac[..., None] * np.asarray(u_filled, dtype=LD)[1:-1, 1:-1, 1:-1, :]
    return y


def extensive_flux(u_filled, eta, fac, h):
    """fac area_d (-b_d du_n/dx_d + cross_d(n)) = -fac area_d tau_nd on every d-face"""
    tau = stress(u_filled, eta, h)
    return [-LD(fac) * LD(h[(d + 1) % 3]) * LD(h[(d + 2) % 3]) * tau[d] for d in range(3)]


# ---------------------------------------------------------------------------------------------------------------------------
# the cases
def _cut(n, cuts):
    edges = [[0] + ([cuts[d]] if cuts[d] and 0 < cuts[d] < n[d] else []) + [n[d]] for d in range(3)]
    return [((x0, y0, z0), (x1 - 1, y1 - 1, z1 - 1))
            for z0, z1 in zip(edges[2][:-1], edges[2][1:]) for y0, y1 in zip(edges[1][:-1], edges[1][1:])
            for x0, x1 in zip(edges[0][:-1], edges[0][1:])]


def _chop(n, m):
    return [((i, j, k), (min(i + m, n[0]) - 1, min(j + m, n[1]) - 1, min(k + m, n[2]) - 1))
            for k in range(0, n[2], m) for j in range(0, n[1], m) for i in range(0, n[0], m)]


PROB_HI = (1.0, 0.5, 0.25)
PROB_HI_ANISO = (2.0, 0.5, 0.25)           # every pair of cell sizes differs on (40, 12, 10)
LAYOUTS = {
    "tile path, one box, partial tiles": dict(n=(40, 12, 10), boxes=_cut((40, 12, 10), (0, 0, 0)), tile=True),
    "tile path, dead tiles": dict(n=(48, 16, 12), boxes=_cut((48, 16, 12), (40, 12, 8)), tile=True),
    "plain path, several boxes": dict(n=(16, 12, 10), boxes=_chop((16, 12, 10), 8), tile=False),
}
TILE_LAYOUTS = [k for k, v in LAYOUTS.items() if v["tile"]]
VISCOSITIES = ("constant", "array")
ETA_CONST = 0.013
FACES = [(d, s) for d in range(3) for s in (0, 1)]
FACE_NAME = {(d, s): "xyz"[d] + ("lo", "hi")[s] for d, s in FACES}


def max_len(boxes):
    return tuple(max(hi[d] - lo[d] + 1 for lo, hi in boxes) for d in range(3))


def z_chunk(len_z):
    """planes a workgroup of the tile kernels marches through (tensor_uni_launch, tensor_cross_terms_sub)"""
    return min(32, max(4, len_z // 8))


def _bc9(per, special=None):
    """all walls Dirichlet; special: {(component, d, side): code}"""
    lo = [PER if per[d] else DIR for _ in range(3) for d in range(3)]
    hi = list(lo)
    for (c, d, s), code in (special or {}).items():
        (lo if s == 0 else hi)[3 * c + d] = code
    return lo, hi


def single_change(face, code, comp):
    """the all-Dirichlet box with one (face, type, component) changed"""
    lo, hi = _bc9((0, 0, 0), {(comp, face[0], face[1]): code})
    return dict(name=f"{FACE_NAME[face]}-{code}-comp{comp}", per=(0, 0, 0), lo=lo, hi=hi, boost=None)


def _bc_sets():
    sets = []
    W = (0, 0, 0)
    for f in FACES:
        d, s = f
        # Dirichlet like every other wall: what singles the face out is its boundary data, three times as large
        lo, hi = _bc9(W)
        sets.append(dict(name=f"{FACE_NAME[f]}-101", per=W, lo=lo, hi=hi, boost=f))
        for code in (NEU, ODD):
            lo, hi = _bc9(W, {(c, d, s): code for c in range(3)})
            sets.append(dict(name=f"{FACE_NAME[f]}-{code}", per=W, lo=lo, hi=hi, boost=None))
    for f in FACES:                     # slip wall: the normal component Dirichlet, the tangential ones Neumann
        d, s = f
        lo, hi = _bc9(W, {(c, d, s): NEU for c in range(3) if c != d})
        sets.append(dict(name=f"{FACE_NAME[f]}-slip", per=W, lo=lo, hi=hi, boost=None))
    d, s = 1, 1                         # symmetry face: the normal component odd, the tangential ones Neumann
    lo, hi = _bc9(W, {(c, d, s): (ODD if c == d else NEU) for c in range(3)})
    sets.append(dict(name="yhi-symmetry", per=W, lo=lo, hi=hi, boost=None))
    per = (0, 1, 0)                     # periodic mixes with walls that differ between lo and hi
    lo, hi = _bc9(per, {**{(c, 0, 1): NEU for c in range(3)}, **{(c, 2, 0): ODD for c in range(3)}})
    sets.append(dict(name="periodic-y", per=per, lo=lo, hi=hi, boost=None))
    per = (1, 0, 1)
    lo, hi = _bc9(per, {(c, 1, 0): NEU for c in range(3)})
    sets.append(dict(name="periodic-xz", per=per, lo=lo, hi=hi, boost=None))
    return sets


BC_SETS = _bc_sets()
BC_BY_NAME = {b["name"]: b for b in BC_SETS}
ALL_DIRICHLET = dict(name="all-101", per=(0, 0, 0), lo=_bc9((0, 0, 0))[0], hi=_bc9((0, 0, 0))[1], boost=None)
MAXORDERS = (2, 3)


def _smooth(X, Y, Z):
    return (np.sin(np.pi * X) * np.cos(2 * np.pi * Y) * np.sin(np.pi * Z) + 0.3 * Z,
            np.cos(3 * X) * np.sin(2 * np.pi * Y) + 0.2 * X * Z,
            0.5 * np.sin(2 * np.pi * (X + Y)) * Z * (1 - Z))


def velocity(n, bcset, seed=11):
    """(nx + 2, ny + 2, nz + 2, 3) float64, Fortran order: the smooth fields of the wall tests of the tensor operator + 0.05 x normal
    noise in the cells; the ghost layer holds the boundary data -- another value on every face and component, varying along the
    face, three times as large on the face bcset["boost"] -- as one global array, images in the periodic directions"""
    rng = np.random.default_rng(seed)
    ax = [(np.arange(-1, n[d] + 1) + 0.5) / n[d] for d in range(3)]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    sm = _smooth(X, Y, Z)
    u = np.zeros(tuple(v + 2 for v in n) + (3,), order="F")
    for c in range(3):
        u[..., c] = sm[c]
    u[1:-1, 1:-1, 1:-1, :] += 0.05 * rng.standard_normal(tuple(n) + (3,))
    for d, s in FACES:
        sl = [slice(None)] * 3
        sl[d] = 0 if s == 0 else n[d] + 1
        for c in range(3):
            val = 0.15 * (1 + 2 * d + s) * (-1.0 if c == 1 else 1.0) + 0.05 * c
            u[tuple(sl) + (c,)] = val + 0.2 * sm[c][tuple(sl)]
    if bcset["boost"] is not None:
        d, s = bcset["boost"]
        sl = [slice(None)] * 3
        sl[d] = 0 if s == 0 else n[d] + 1
        u[tuple(sl)] *= 3.0
    for d in range(3):
        if bcset["per"][d]:
            lo = [slice(None)] * 3; hi = [slice(None)] * 3; slo = [slice(None)] * 3; shi = [slice(None)] * 3
            lo[d], slo[d], hi[d], shi[d] = 0, n[d], n[d] + 1, 1
            u[tuple(lo)] = u[tuple(slo)]
            u[tuple(hi)] = u[tuple(shi)]
    return u


def viscosity(n, kind, per=(0, 0, 0), seed=23):
    """three face arrays (.., 1), float64: the constant 0.013, or values between 0.01 and 0.02 (ratio > 1.8)"""
    rng = np.random.default_rng(seed)
    eta = []
    for d in range(3):
        shape = tuple(n[e] + (e == d) for e in range(3)) + (1,)
        if kind == "constant":
            e = np.full(shape, ETA_CONST, order="F")
        else:
            e = np.asfortranarray(0.01 * (1.0 + rng.random(shape)))
            if per[d]:
                lo = [slice(None)] * 3; hi = [slice(None)] * 3
                lo[d], hi[d] = 0, n[d]
                e[tuple(hi)] = e[tuple(lo)]
        eta.append(e)
    return eta


def a_coefficient(n):
    ax = [(np.arange(n[d]) + 0.5) / n[d] for d in range(3)]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    return np.asfortranarray((1.0 + 0.2 * np.cos(2 * np.pi * X) * np.cos(np.pi * Z))[..., None])


FORMS = {"explicit": (0.0, -1.0, False), "implicit": (1.0, 0.004, True)}       # (a, b, with the a-array): HASA off / on


def cell_sizes(n, prob_hi):
    return tuple(prob_hi[d] / n[d] for d in range(3))


@functools.lru_cache(maxsize=None)
def case(layout, visc, bcname, maxorder, form="explicit", prob_hi=PROB_HI):
    """inputs (float64) and reference results (longdouble) of one case; computed once, shared and left unchanged by the tests"""
    L = LAYOUTS[layout]
    n = L["n"]
    bcset = ALL_DIRICHLET if bcname == ALL_DIRICHLET["name"] else BC_BY_NAME[bcname]
    return build(n, visc, bcset, maxorder, form, prob_hi, boxes=L["boxes"])


def build(n, visc, bcset, maxorder, form="explicit", prob_hi=PROB_HI, boxes=None, fac=1.0):
    a, b, with_a = FORMS[form]
    h = cell_sizes(n, prob_hi)
    u = velocity(n, bcset)
    eta = viscosity(n, visc, bcset["per"])
    acoef = a_coefficient(n) if with_a else None
    uf = fill_ghosts(u, u, bcset["per"], bcset["lo"], bcset["hi"], maxorder, True)
    y = apply(uf, eta, a, b, acoef, h)
    flux = extensive_flux(uf, eta, fac, h)
    for arr in [u, uf, y] + eta + flux + ([acoef] if with_a else []):
        arr.setflags(write=False)
    return dict(n=n, h=h, prob_hi=prob_hi, boxes=boxes, bc=bcset, maxorder=maxorder, a=a, b=b, acoef=acoef, u=u, eta=eta, u_filled=uf,
                y=y, flux=flux, visc=visc)
