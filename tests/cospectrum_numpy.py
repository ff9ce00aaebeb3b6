"""numpy yardstick of the co-spectra, the k^2-weighted power, the skew-symmetric nonlinear term and the spectral energy budget
(include/iamrx.h: iamrx_mf_cospectrum / iamrx_mf_spectrum_k2 / iamrx_convective_term / iamrx_ns_spectral_budget; kernels in
iamr_amd/csrc/k_spectrum.hip and k_convect.hip).  Built on spectrum_numpy: the transform F = np.fft.fftn / N, the shells, eps_of.

Co-spectrum.  C_ab(s) = math.fsum over the shell of Re(F_a conj F_b).
  Bound, derived and not tuned.  The library transforms Z = a + i b once, ||Z||^2 = Pt_a + Pt_b (Pt: the power summed over all shells);
  a transform with ||dZ||_2 <= eps ||Z||_2, eps = eps_of(N), gives dF_a(m) = (dZ(m) + conj dZ(-m)) / 2 and dF_b(m) = (dZ(m) -
  conj dZ(-m)) / (2 i), so over a shell that is symmetric under m -> -m their 2-norms alpha, beta obey alpha^2 + beta^2 = ||dZ||_shell^2
  <= eps^2 (Pt_a + Pt_b) (parallelogram law).  d Re(F_a conj F_b) = Re(dF_a conj F_b) + Re(F_a conj dF_b) + Re(dF_a conj dF_b) summed
  over the shell is at most alpha sqrt(P_b(s)) + beta sqrt(P_a(s)) + alpha beta <= sqrt(alpha^2 + beta^2) sqrt(P_a(s) + P_b(s)) +
  (alpha^2 + beta^2) / 2 by Cauchy-Schwarz, hence
    |dC(s)| <= eps sqrt((P_a(s) + P_b(s)) (Pt_a + Pt_b)) + eps^2 (Pt_a + Pt_b) / 2 + count(s) 2^-53 (P_a(s) + P_b(s)) / 2,
  the last term for adding count(s) terms of magnitude <= (|F_a|^2 + |F_b|^2) / 2 in any order.  Two plain transforms obey it as well.
  The powers P_a, P_b that the packed form yields beside C obey the bound of spectrum_numpy with P_tot replaced by Pt_a + Pt_b
  (power_bound_packed); iamrx_mf_cospectrum's are tested against spectrum_numpy's own, narrower bound.

k^2-weighted power.  W(s) = math.fsum of k(m)^2 |F(m)|^2, k(m)^2 = (2 pi / L_max)^2 kappa(m)^2, kappa^2 formed as the shell index forms it.
  Bound: the library's weight w' = (c kappa^2) with c = (2 pi / L_max) squared carries four roundings (the division, the square, the
  product with kappa^2, the product with |F|^2): |w' - w| <= 4 u w (1 + O(u)), u = 2^-53.  The bound of spectrum_numpy bounds the sum of
  the ABSOLUTE errors of |F|^2 over the shell (its Cauchy-Schwarz step is applied to absolute values), so with k2max(s) the largest
  k^2 of the shell
    |dW(s)| <= k2max(s) (1 + 4 u) (2 eps sqrt(P(s) P_tot) + eps^2 P_tot) + (4 + count(s)) u W(s).

Nonlinear term.  With h_d = 0.5 / dx_d, N_i = 0.5 sum_d (a_d + b_d), a_d = u_d ((u_i(+e_d) - u_i(-e_d)) h_d),
  b_d = (u_d(+e_d) u_i(+e_d) - u_d(-e_d) u_i(-e_d)) h_d; periodic data by np.roll, ghost-filled data by slices.
  Bound per cell: gamma_k times the sum of the absolute values of the six terms taken BEFORE their differences cancel, i.e.
    M_i = 0.5 sum_d h_d [ |u_d| (|u_i(+e_d)| + |u_i(-e_d)|) + |u_d(+e_d) u_i(+e_d)| + |u_d(-e_d) u_i(-e_d)| ],
  with k = 8 the number of roundings on the longest path: dx_d and h_d (2), difference, product with h_d, product with u_d (3), and the
  three additions (a_0 + b_0), + (a_1 + b_1), + (a_2 + b_2) (3); the factor 0.5 is exact.  gamma_k = k u / (1 - k u).
  sum_x u_i N_i vanishes identically for the exact N of any periodic u, so |sum u_i N_i| of a computed N is bounded by
  sum |u_i| gamma_k M_i plus u sum |u_i N_i| for the products (the sum itself is taken with math.fsum).

Budget of a level, composed from a read-back state S: E = (P_u + P_v + P_w) / 2, T = -(C_uN0 + C_vN1 + C_wN2), D = visc (W_u + W_v +
  W_w), F = C_uf0 + C_vf1 + C_wf2; the bounds are the sums of the bounds of the parts, the powers with the packed form's bound, T with
  one more term for the rounding of N itself, |C_{u dN}(s)| <= sqrt(P_u(s) mean(dN^2)) <= sqrt(P_u(s) mean((gamma_k M)^2)), and three
  roundings of the combination."""
import math
import numpy as np
import spectrum_numpy as SN

U = 2.0 ** -53
K_ROUNDINGS = 8
GAMMA = K_ROUNDINGS * U / (1.0 - K_ROUNDINGS * U)


def _sum_shells(v, s, nbins):
    order = np.argsort(s.ravel(), kind="stable")
    count = np.bincount(s.ravel(), minlength=nbins).astype(np.int64)
    ends = np.cumsum(count)
    v = v.ravel()
    return np.array([math.fsum(v[order[e - c:e]]) for c, e in zip(count, ends)]), count


def cospectrum_from(Fa, Fb, s, nbins):
    """-> (C, P_a, P_b, count) from two transforms (already divided by N)"""
    C, count = _sum_shells((Fa * np.conj(Fb)).real, s, nbins)
    Pa, _ = SN.shell_sums(Fa, s, nbins)
    Pb, _ = SN.shell_sums(Fb, s, nbins)
    return C, Pa, Pb, count


def cospectrum_reference(a, b, L):
    s, nbins, _ = SN.shell_index(a.shape, L)
    N = float(a.size)
    return cospectrum_from(np.fft.fftn(a) / N, np.fft.fftn(b) / N, s, nbins)


def cospectrum_packed(a, b, L, transform=SN.radix2):
    """the library's form on the CPU: ONE transform of Z = a + i b, the mode read with its mirror mode"""
    s, nbins, _ = SN.shell_index(a.shape, L)
    Z = transform(a + 1j * b)
    M = Z
    for ax in range(3):
        M = np.roll(np.flip(M, ax), 1, ax)          # index (n - i) % n
    C, count = _sum_shells(0.5 * (Z * M).imag, s, nbins)
    Pa, _ = _sum_shells(0.25 * np.abs(Z + np.conj(M)) ** 2, s, nbins)
    Pb, _ = _sum_shells(0.25 * np.abs(Z - np.conj(M)) ** 2, s, nbins)
    return C, Pa, Pb, count


def cospectrum_bound(Pa, Pb, count, N):
    eps, Pt = SN.eps_of(N), math.fsum(Pa) + math.fsum(Pb)
    return eps * np.sqrt((Pa + Pb) * Pt) + eps * eps * Pt / 2.0 + count * U * (Pa + Pb) / 2.0


def power_bound_packed(P, Pt_pair, count, N):
    """spectrum_numpy.bound with the 2-norm of the packed pair in place of the field's own"""
    eps = SN.eps_of(N)
    return 2.0 * eps * np.sqrt(P * Pt_pair) + eps * eps * Pt_pair + count * U * P


def k2_of(n, L):
    """k(m)^2 (n_x, n_y, n_z), kappa^2 formed as the shell index forms it"""
    Lmax = max(float(v) for v in L)
    r = [Lmax / float(v) for v in L]
    a = [SN.mode_numbers(n[d]).astype(np.float64) * r[d] for d in range(3)]
    ax, ay, az = a[0][:, None, None], a[1][None, :, None], a[2][None, None, :]
    k0 = 2.0 * math.pi / Lmax
    return (k0 * k0) * ((ax * ax + ay * ay) + az * az)


def k2_reference(f, L):
    """-> (W, P, count, k2max per shell)"""
    s, nbins, _ = SN.shell_index(f.shape, L)
    F = np.fft.fftn(f) / float(f.size)
    k2 = np.broadcast_to(k2_of(f.shape, L), f.shape)
    W, count = _sum_shells(k2 * (F.real * F.real + F.imag * F.imag), s, nbins)
    P, _ = SN.shell_sums(F, s, nbins)
    k2max = np.zeros(nbins)
    np.maximum.at(k2max, s.ravel(), k2.ravel())
    return W, P, count, k2max


def k2_bound(W, P, count, k2max, N, Pt=None):
    """Pt: the squared 2-norm the transform's error is relative to (default: the field's own; the packed pair's for the budget)"""
    eps = SN.eps_of(N)
    Pt = math.fsum(P) if Pt is None else Pt
    return k2max * (1.0 + 4.0 * U) * (2.0 * eps * np.sqrt(P * Pt) + eps * eps * Pt) + (4.0 + count) * U * W


def convective_reference(V, dx, ghost=False):
    """V (.., .., .., 3): periodic data (ghost False: neighbours by np.roll) or data with one filled ghost layer (ghost True: the result
    covers the interior) -> (N, M) of the same shape (.., 3): the term and the sum of absolute values its bound multiplies"""
    h = [0.5 / float(dx[d]) for d in range(3)]
    inner = (slice(1, -1),) * 3

    def nb(d, sgn):
        if not ghost:
            return np.roll(V, -sgn, axis=d)
        sl = [slice(1, -1)] * 3
        sl[d] = slice(2, None) if sgn > 0 else slice(0, -2)
        return V[tuple(sl)]

    c = V[inner] if ghost else V
    N, M = np.zeros(c.shape), np.zeros(c.shape)
    for i in range(3):
        t, m = [], []
        for d in range(3):
            hi, lo = nb(d, +1), nb(d, -1)
            a = c[..., d] * ((hi[..., i] - lo[..., i]) * h[d])
            b = (hi[..., d] * hi[..., i] - lo[..., d] * lo[..., i]) * h[d]
            t.append(a + b)
            m.append(h[d] * (np.abs(c[..., d]) * (np.abs(hi[..., i]) + np.abs(lo[..., i])) + np.abs(hi[..., d] * hi[..., i]) + np.abs(lo[..., d] * lo[..., i])))
        N[..., i] = 0.5 * ((t[0] + t[1]) + t[2])
        M[..., i] = 0.5 * ((m[0] + m[1]) + m[2])
    return N, M


def energy_identity(V, N, M):
    """-> (sum_x u_i N_i by math.fsum, its bound)"""
    return math.fsum((V * N).ravel()), GAMMA * math.fsum((np.abs(V) * M).ravel()) + U * math.fsum(np.abs(V * N).ravel())


def budget_reference(S, L, visc, f=None):
    """S (n, >= 3) the velocity read back, f (n, 3) the forcing's acceleration or None -> dict of E, T, D, F, count and their bounds bE .."""
    n, Nc = S.shape[:3], float(S[..., 0].size)
    dx = [float(L[d]) / n[d] for d in range(3)]
    V = np.ascontiguousarray(S[..., :3])
    Nl, M = convective_reference(V, dx)
    nb = SN.shell_index(n, L)[1]
    out = {k: np.zeros(nb) for k in ("E", "T", "D", "F", "bE", "bT", "bD", "bF")}
    for i in range(3):
        u = np.ascontiguousarray(V[..., i])
        C, Pu, Pn, cnt = cospectrum_reference(u, np.ascontiguousarray(Nl[..., i]), L)
        Pt = math.fsum(Pu) + math.fsum(Pn)
        W, _, _, k2max = k2_reference(u, L)
        out["E"] += 0.5 * Pu
        out["bE"] += 0.5 * power_bound_packed(Pu, Pt, cnt, Nc)
        out["T"] -= C
        out["bT"] += cospectrum_bound(Pu, Pn, cnt, Nc) + np.sqrt(Pu * float(np.mean((GAMMA * M[..., i]) ** 2)))
        out["D"] += visc * W
        out["bD"] += visc * k2_bound(W, Pu, cnt, k2max, Nc, Pt)
        if f is not None:
            Cf, _, Pf, _ = cospectrum_reference(u, np.ascontiguousarray(f[..., i]), L)
            out["F"] += Cf
            out["bF"] += cospectrum_bound(Pu, Pf, cnt, Nc)
        out["count"] = cnt
    for k in ("E", "T", "D", "F"):
        out["b" + k] += 3.0 * U * np.abs(out[k])
    return out
