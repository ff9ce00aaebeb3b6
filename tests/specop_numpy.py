"""numpy yardstick of the way back from mode space (include/iamrx.h: iamrx_mf_noise / iamrx_mf_filter / iamrx_mf_solenoidal /
iamrx_mf_synthesize; iamr_amd/csrc/k_spectrum.hip), in the notation of spectrum_numpy.py, whose shell index it reuses.

For a field f on n = (n_x, n_y, n_z) cells, N = n_x n_y n_z, side lengths L, L_max = max L, r_d = L_max / L_d, k0 = 2 pi / L_max:
  F = fftn(f) / N, signed mode numbers m_d, kappa^2 = ((m_x r_x)^2 + (m_y r_y)^2) + (m_z r_z)^2, k_d = k0 m_d r_d, dx_d = L_d / n_d;
  filter      f' = N ifftn(G F) with Delta = pi / (k0 kc):  0 G = 1;  1 G = [kappa^2 <= kc^2];  2 G = exp(-kappa^2 pi^2 / (24 kc^2));
              3 G = prod_d sinc(pi m_d r_d / (2 kc)), sinc(x) = sin(x) / x, sinc(0) = 1;
  projection  u(m) <- u(m) - q (q . u(m)) / |q|^2 where |q|^2 > 0;  exact q_d = k_d, centred q_d = sin(2 pi m_d / n_d) / dx_d, and
              q_d = 0 at m_d = -n_d / 2 in both forms (the Nyquist rule).  The centred sine is taken of the angle reduced to
              [-pi / 2, pi / 2] through the integer m (sin(pi - x) = sin(x)), so that its relative error stays a few 2^-53 also next to
              the Nyquist mode, where sin(2 pi m / n) is small and the rounding of the angle would otherwise be n times larger;
  noise       include/iamrx.h's counter-based generator in uint64 (wrapping) arithmetic, exact in double;
  synthesis   noise for c = 0, 1, 2 -> F -> projection -> E_now(s) = fsum over the shell of (|F_u|^2 + |F_v|^2 + |F_w|^2) / 2 ->
              a(s) = sqrt(E_target(s) / E_now(s)) (0 for s = 0 and where E_now = 0) -> a F -> back.

The bounds, derived and not tuned.  u = 2^-53.  One transform errs by ||dF||_2 <= eps1 ||F||_2, eps1 = 8 log2(N) u (spectrum_numpy.py:
Higham's FFT bound with twiddles good to an ulp or two); all norms are 2-norms over the cells (and the components of a vector).

  filter      A side makes two transforms and multiplies by |G| <= 1 in between: (2 eps1 + its error in G) ||f||.  The library takes
              each per-axis factor from a table made in extended precision and rounded once (within u (1 + 2^-10) of the true factor:
              glibc's expl / sinl are good to 1 ulp OF THE EXTENDED FORMAT, glibc manual, "Known Maximum Errors in Math Functions",
              x86_64 column) and multiplies three of them (2 roundings): <= 5.1 u absolute since every factor is <= 1.  numpy's double
              exp and sin are good to 1 ulp = 2 u in the same table of the manual; the Gaussian's argument carries 4 roundings, which
              exp(-x) turns into <= 4 u x exp(-x) <= 1.5 u; a sinc factor errs by <= 2 u (sin) + 3 u (the argument's three roundings
              times |cos|) + u (the division), three factors and two products: <= 20 u.  c_G = 32 covers both sides:
                ||got - ref|| <= (4 eps1 + c_G u) ||f||.
  projection  P = I - q q^T / |q|^2 is an orthogonal projector for real q, ||P|| = 1.  Evaluating it costs a three-term dot product
              (3 u |q| |u|), a division, a product and a difference (3 u): 6 u |u|; a table entry of q is within u (1 + 2^-10) of the
              true value in the library and within 5 u in numpy (angle 2 roundings, times x cot x <= 1 after the reduction, sin 2 u, the
              division u), and dq changes P by <= 2 |dq| / |q|: c_P = 2 (6 + 2 * 5) = 32 for both sides together:
                ||got - ref|| <= (4 eps1 + c_P u) ||f||,   and one side alone: ||got - exact|| <= (2 eps1 + c_P u) ||f||.
  divergence  of a centred-projected field, D = sum_d (f(x + e_d) - f(x - e_d)) (0.5 / dx_d): the symbol of a difference is
              i sin(2 pi m_d / n_d) / dx_d = i q_d, so D vanishes on the exactly projected field (also in the Nyquist planes, where the
              symbol is 0 and the rule leaves the mode alone) and sees only the error e of the field: |symbol_d| <= 1 / dx_d and
              Cauchy-Schwarz over d give ||D e|| <= sqrt(sum_d dx_d^-2) ||e||; the differences themselves round by <= 3 u |u_d| / dx_d
              per direction and cell:
                rms(D) <= sqrt(sum_d dx_d^-2) (2 eps1 + c_P u) ||f|| / sqrt(N) + 3 u sum_d max|u_d| / dx_d.
  the exact projection applied to a centred-projected field u (q_c . u = 0) still removes, mode by mode, k (k . u) / |k|^2, of norm
              |k . u| / |k|: cross_removed() sums it.  It vanishes only where q_c is parallel to k.
  synthesis   with Pn = sum over the three components of mean(noise^2), P_G(s) = 2 E_now(s):
              A  projected modes, both sides: ||dG|| <= 2 eA sqrt(Pn), eA = eps1 + c_P u / 2;
              B  the shell sums inherit it as in spectrum_numpy: dP(s) <= 2 (2 eA) sqrt(P_G(s) Pn) + (2 eA)^2 Pn + 3 count(s) u P_G(s),
                 and a = sqrt(E_target / E_now) gives da / a <= dP / (2 P_G) + 2 u (division and root);
              C  ||d(a G)|| <= a_max ||dG|| + sqrt(sum_s (da / a)^2 2 E_target(s));
              D  the transforms back, both sides: 2 eps1 sqrt(2 E_tot), E_tot = sum_s E_target(s).
              ||got - ref|| / sqrt(N) <= a_max 2 eA sqrt(Pn) + sqrt(sum_s (dP / (2 P_G) + 2 u)^2 2 E_target) + 2 eps1 sqrt(2 E_tot);
              one side alone (against the exact field of its own noise): the same with eA, eps1 in place of 2 eA, 2 eps1.
              The spectrum of the result, measured by mf_spectrum (eps = 2 eps1, spectrum_numpy.bound), is E_target within
                shell_bound(2 E_target, count, eps_meas + e_side / sqrt(2 E_tot)) / 2,
              the measurement's eps widened by the one-sided relative error of the field.

A sharp cut-off within 1e-9 of a mode's kappa is asserted away (and spectrum_numpy asserts the shell boundaries away): a tie must never
decide a test."""
import math
import numpy as np
import spectrum_numpy as SN

U = 2.0 ** -53
C_G = 32.0
C_P = 32.0
M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15


def eps1(N):
    return 8.0 * math.log2(N) * U


# ------------------------------------------------------------------------------------------------------------------ noise
def _mix(z):
    """z: uint64 array (wrapping)"""
    z = z + np.uint64(GOLD)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def noise(n, seed, ncomp=1):
    """-> (n_x, n_y, n_z, ncomp) float64, component c at global cell index o = i + n_x (j + n_y k)"""
    n = tuple(int(v) for v in n)
    N = n[0] * n[1] * n[2]
    out = np.empty(n + (ncomp,))
    o = np.arange(N, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for c in range(ncomp):
            key = _mix(np.array([(int(seed) ^ (((c + 1) * GOLD) & M64)) & M64], dtype=np.uint64))
            h = _mix(key + o)
            v = ((h >> np.uint64(12)).astype(np.float64) + 0.5) * 2.0 ** -52 - 0.5
            out[..., c] = v.reshape(n[::-1]).transpose(2, 1, 0)          # o runs with x fastest
    return out


# ------------------------------------------------------------------------------------------------------------------ mode tables
def _ratios(L):
    Lmax = max(float(v) for v in L)
    return [Lmax / float(v) for v in L], Lmax


def _axes(vals):
    return vals[0][:, None, None], vals[1][None, :, None], vals[2][None, None, :]


def kappa2(n, L):
    r, _ = _ratios(L)
    ax, ay, az = _axes([SN.mode_numbers(n[d]).astype(np.float64) * r[d] for d in range(3)])
    return (ax * ax + ay * ay) + az * az


def filter_G(n, L, kind, kc):
    r, _ = _ratios(L)
    if kind == 0:
        return np.ones(tuple(n))
    if kind == 1:
        k2 = kappa2(n, L)
        assert float(np.min(np.abs(np.sqrt(k2) - kc))) > SN.TIE, (n, L, kc)
        return np.where(k2 <= kc * kc, 1.0, 0.0)
    if kind == 2:
        return np.exp(-kappa2(n, L) * (math.pi * math.pi) / (24.0 * kc * kc))
    if kind == 3:
        fac = []
        for d in range(3):
            x = math.pi * SN.mode_numbers(n[d]).astype(np.float64) * r[d] / (2.0 * kc)
            fac.append(np.where(x == 0.0, 1.0, np.sin(x) / np.where(x == 0.0, 1.0, x)))
        gx, gy, gz = _axes(fac)
        return (gx * gy) * gz
    raise ValueError(kind)


def wave_vector(n, L, wavenumber):
    """q_d on the axes (three broadcastable arrays); wavenumber 0 exact, 1 centred; 0 at m_d = -n_d / 2"""
    q = []
    for d in range(3):
        nd = int(n[d])
        m = SN.mode_numbers(nd)
        if wavenumber == 0:
            v = 2.0 * math.pi * m.astype(np.float64) / float(L[d])
        else:
            mm = np.where(4 * m > nd, nd // 2 - m, np.where(4 * m < -nd, -(nd // 2) - m, m))
            v = np.sin(2.0 * math.pi * mm.astype(np.float64) / nd) / (float(L[d]) / nd)
        v[m == -(nd // 2)] = 0.0
        q.append(v)
    return _axes(q)


def project_modes(F, q):
    """F: (3, n_x, n_y, n_z) complex -> the same, projected"""
    qx, qy, qz = q
    q2 = (qx * qx + qy * qy) + qz * qz
    dot = (qx * F[0] + qy * F[1]) + qz * F[2]
    c = np.where(q2 != 0.0, dot / np.where(q2 != 0.0, q2, 1.0), 0.0)
    return np.stack([F[0] - qx * c, F[1] - qy * c, F[2] - qz * c])


def cross_removed(f, L, wavenumber_other):
    """f (n, 3): what the projection of the OTHER wavenumber form still removes from f, sqrt(sum_m |q . F|^2 / |q|^2) N^(1/2) -- the 2-norm
    over cells and components of (f - other projection of f) in exact arithmetic"""
    n = f.shape[:3]
    F = np.stack([np.fft.fftn(f[..., c]) for c in range(3)]) / float(f[..., 0].size)
    qx, qy, qz = wave_vector(n, L, wavenumber_other)
    q2 = (qx * qx + qy * qy) + qz * qz
    dot = (qx * F[0] + qy * F[1]) + qz * F[2]
    t = np.where(q2 != 0.0, (dot.real ** 2 + dot.imag ** 2) / np.where(q2 != 0.0, q2, 1.0), 0.0)
    return math.sqrt(math.fsum(t.ravel()) * f[..., 0].size)


# ------------------------------------------------------------------------------------------------------------------ transforms
def np_fwd(f):
    return np.fft.fftn(f) / float(f.size)


def np_inv(F):
    return np.fft.ifftn(F) * float(F.size)


def r2_fwd(f):
    return SN.radix2(f)


def r2_inv(F):
    """conj(FFT(conj(N F))) / N through the independent radix-2 transform"""
    return np.conj(SN.radix2(np.conj(F))) * float(F.size)


# ------------------------------------------------------------------------------------------------------------------ references
def filter_reference(f, L, kind, kc, fwd=np_fwd, inv=np_inv):
    """f (n_x, n_y, n_z) -> filtered"""
    return inv(filter_G(f.shape, L, kind, kc) * fwd(f)).real


def solenoidal_reference(f, L, wavenumber, fwd=np_fwd, inv=np_inv):
    """f (n, 3) -> (n, 3)"""
    F = project_modes(np.stack([fwd(f[..., c]) for c in range(3)]), wave_vector(f.shape[:3], L, wavenumber))
    return np.stack([inv(F[c]).real for c in range(3)], axis=-1)


def centred_divergence(f, L):
    """sum_d (f_d(x + e_d) - f_d(x - e_d)) (0.5 / dx_d), periodic"""
    n = f.shape[:3]
    return sum((np.roll(f[..., d], -1, axis=d) - np.roll(f[..., d], 1, axis=d)) * (0.5 / (float(L[d]) / n[d])) for d in range(3))


def synth_reference(n, L, seed, E_target, wavenumber, fwd=np_fwd, inv=np_inv):
    """-> (field (n, 3), info: Pn, P_G (nbins,), count, a)"""
    n = tuple(int(v) for v in n)
    w = noise(n, seed, 3)
    s, nbins, _ = SN.shell_index(n, L)
    E_target = np.asarray(E_target, dtype=np.float64)
    assert E_target.shape == (nbins,)
    F = project_modes(np.stack([fwd(w[..., c]) for c in range(3)]), wave_vector(n, L, wavenumber))
    sums = [SN.shell_sums(F[c], s, nbins) for c in range(3)]
    P_G = (sums[0][0] + sums[1][0]) + sums[2][0]
    count = sums[0][1]
    E_now = 0.5 * P_G
    ok = (E_now > 0.0) & (np.arange(nbins) > 0)
    if np.any((E_target > 0.0) & ~ok & (np.arange(nbins) > 0)):
        raise ValueError("the target asks for energy in a shell the noise leaves empty")
    a = np.where(ok, np.sqrt(E_target / np.where(ok, E_now, 1.0)), 0.0)
    field = np.stack([inv(a[s] * F[c]).real for c in range(3)], axis=-1)
    Pn = float(sum(np.mean(w[..., c] ** 2) for c in range(3)))
    return field, dict(Pn=Pn, P_G=P_G, count=count, a=a, nbins=nbins)


# ------------------------------------------------------------------------------------------------------------------ bounds
def norm2(a):
    return math.sqrt(math.fsum((np.asarray(a, dtype=np.float64) ** 2).ravel()))


def filter_bound(f):
    """on ||got - ref||_2 of one filtered component f (n_x, n_y, n_z)"""
    return (4.0 * eps1(f.size) + C_G * U) * norm2(f)


def filter_eps(N):
    return 4.0 * eps1(N) + C_G * U


def projection_bound(f):
    """on ||got - ref||_2 over cells and components of a projected vector f (n, 3)"""
    return (4.0 * eps1(f[..., 0].size) + C_P * U) * norm2(f)


def divergence_bound(f_in, f_out, L):
    """on the rms over cells of the centred divergence of f_out = the centred projection of f_in (both (n, 3))"""
    n = f_in.shape[:3]
    N = f_in[..., 0].size
    dx = [float(L[d]) / n[d] for d in range(3)]
    return (math.sqrt(sum(1.0 / (h * h) for h in dx)) * (2.0 * eps1(N) + C_P * U) * norm2(f_in) / math.sqrt(N)
            + 3.0 * U * sum(float(np.max(np.abs(f_out[..., d]))) / dx[d] for d in range(3)))


def shell_bound(P, count, eps, terms=1):
    """spectrum_numpy.bound with a free eps; terms: the components added into P"""
    Ptot = math.fsum(P)
    return 2.0 * eps * np.sqrt(P * Ptot) + eps * eps * Ptot + terms * count * U * P


def synth_field_bound(E_target, info, N, sides=2):
    """on sqrt(sum over cells and components of (got - ref)^2 / N); sides = 1: one side against the exact field of its own noise"""
    E_target = np.asarray(E_target, dtype=np.float64)
    eA, e1 = sides * (eps1(N) + 0.5 * C_P * U), sides * eps1(N)
    Pn, P_G, count, a = info["Pn"], info["P_G"], info["count"], info["a"]
    live = a > 0.0
    dP = 2.0 * eA * np.sqrt(P_G * Pn) + eA * eA * Pn + 3.0 * count * U * P_G
    rel = np.where(live, dP / (2.0 * np.where(live, P_G, 1.0)), 0.0) + 2.0 * U
    assert float(rel.max()) < 1e-6          # first order holds
    Etot = math.fsum(E_target)
    return float(a.max()) * eA * math.sqrt(Pn) + math.sqrt(math.fsum(rel * rel * 2.0 * E_target)) + e1 * math.sqrt(2.0 * Etot)


def synth_divergence_bound(E_target, info, f_out, L):
    """on the rms of the centred divergence of a synthesised field f_out (n, 3): the divergence bound with the one-sided error of the
    synthesis (an rms already) in place of the projection's"""
    n = f_out.shape[:3]
    dx = [float(L[d]) / n[d] for d in range(3)]
    return (math.sqrt(sum(1.0 / (h * h) for h in dx)) * synth_field_bound(E_target, info, f_out[..., 0].size, sides=1)
            + 3.0 * U * sum(float(np.max(np.abs(f_out[..., d]))) / dx[d] for d in range(3)))


def synth_spectrum_bound(E_target, info, N):
    """on |E_measured(s) - E_target(s)| per shell, E_measured = (P_u + P_v + P_w) / 2 of mf_spectrum"""
    E_target = np.asarray(E_target, dtype=np.float64)
    Etot = math.fsum(E_target)
    eps = SN.eps_of(N) + synth_field_bound(E_target, info, N, sides=1) / math.sqrt(2.0 * Etot)
    return 0.5 * shell_bound(2.0 * E_target, info["count"], eps, terms=3)
