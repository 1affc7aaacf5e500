"""numpy restatement of the two embedders (test infrastructure, like permuto_ref.py): the real spherical harmonics from their closed
form, their analytic Jacobian and the bound polynomial M_c, and the frequency embedding's forward / backward / double backward.
Every function works in the dtype it is asked for (``np.float64``: the reference values; ``np.float32``: the twin).

    Y_l^m(x, y, z) = s_m K_l^|m| Q_l^|m|(z) { Re (x + iy)^m, m > 0;  1, m = 0;  Im (x + iy)^|m|, m < 0 },  column l^2 + l + m
    Q_l^a = d^a/dz^a P_l(z),  K_l^a = sqrt((2l + 1) / (4 pi) (l - a)! / (l + a)!),  s_0 = 1,  s_m = (-1)^m sqrt(2)

Written from the definition and independent of tools/gen_sh_basis.py (monomial sums, not Horner tables; binomial sums, not the power
recurrence), so that the two check each other."""
import math
from fractions import Fraction

import numpy as np


# ---- spherical harmonics ----------------------------------------------------------------------------------------------------------
def _legendre(l):
    """{power: Fraction} of P_l"""
    return {l - 2 * k: Fraction((-1) ** k * math.comb(l, k) * math.comb(2 * l - 2 * k, l), 2 ** l) for k in range(l // 2 + 1)}


def _dz(poly):
    return {p - 1: c * p for p, c in poly.items() if p > 0}


def _scale(l, a):
    k = math.sqrt((2 * l + 1) / (4 * math.pi) * math.factorial(l - a) / math.factorial(l + a))
    return k if a == 0 else (-1) ** a * math.sqrt(2.0) * k


def zpoly(l, a, order=0, perturb=None):
    """[(power, coefficient)] of s K_l^a d^order/dz^order Q_l^a(z), highest power first.  perturb = (l, a, term, rel[, order]): that term's
    coefficient of the polynomial of that (l, a) and order (default 0: the value table; 1: the z-derivative table) is multiplied by 1 + rel"""
    q = _legendre(l)
    for _ in range(a + order):
        q = _dz(q)
    out = [(p, float(q[p]) * _scale(l, a)) for p in sorted(q, reverse=True)]
    if perturb is not None and tuple(perturb[:2]) == (l, a) and order == (perturb[4] if len(perturb) > 4 else 0):
        p, c = out[perturb[2]]
        out[perturb[2]] = (p, c * (1.0 + perturb[3]))
    return out


def _polyval(terms, z, absolute=False):
    acc = np.zeros_like(z)
    for p, c in terms:
        acc = acc + (z.dtype.type(abs(c)) * np.abs(z) ** p if absolute else z.dtype.type(c) * z ** p)
    return acc


def _re_im(x, y, a, absolute=False):
    """Re and Im of (x + iy)^a as binomial sums (absolute: every monomial by its absolute value)"""
    re, im = np.zeros_like(x), np.zeros_like(x)
    if a < 0:
        return re, im
    for k in range(a + 1):
        if absolute:
            t = x.dtype.type(math.comb(a, k)) * np.abs(x) ** (a - k) * np.abs(y) ** k
        else:
            t = x.dtype.type(math.comb(a, k) * (-1) ** (k // 2)) * x ** (a - k) * y ** k
        if k % 2 == 0:
            re = re + t
        else:
            im = im + t
    return re, im


def sh_all(xyz, degree, dtype=np.float64, absolute=False, perturb=None):
    """(Y [B, C^2], J [B, 3, C^2]) of the given degree; absolute: the bound polynomials M_c of both (every coefficient and variable
    replaced by its absolute value: an upper bound of the sum of the absolute monomial terms)"""
    p = np.asarray(xyz).astype(dtype)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    B, C2 = p.shape[0], degree * degree
    Y, J = np.zeros((B, C2), dtype), np.zeros((B, 3, C2), dtype)
    sgn = 1.0 if absolute else -1.0
    for l in range(degree):
        for a in range(l + 1):
            q = _polyval(zpoly(l, a, 0, perturb), z, absolute)
            qz = _polyval(zpoly(l, a, 1, perturb), z, absolute) if a < l else np.zeros_like(z)
            re, im = _re_im(x, y, a, absolute)
            pre, pim = _re_im(x, y, a - 1, absolute)
            c = l * l + l
            if a == 0:
                Y[:, c], J[:, 2, c] = q, qz
                continue
            aq = dtype(a) * q
            Y[:, c + a], J[:, 0, c + a], J[:, 1, c + a], J[:, 2, c + a] = q * re, aq * pre, dtype(sgn) * aq * pim, qz * re
            Y[:, c - a], J[:, 0, c - a], J[:, 1, c - a], J[:, 2, c - a] = q * im, aq * pim, aq * pre, qz * im
    return Y, J


def sh(xyz, degree, dtype=np.float64, perturb=None):
    return sh_all(xyz, degree, dtype, perturb=perturb)[0]


def sh_jacobian(xyz, degree, dtype=np.float64):
    return sh_all(xyz, degree, dtype)[1]


def sh_bound(xyz, degree):
    """(M of the values [B, C^2], M of the derivatives [B, 3, C^2]) in fp64"""
    return sh_all(xyz, degree, np.float64, absolute=True)


def sh_backward(g, xyz, degree, dtype=np.float64):
    """dL/dx [B, 3] = sum_c g[b, c] dY_c/dx"""
    return np.einsum("bc,bdc->bd", np.asarray(g).astype(dtype), sh_jacobian(xyz, degree, dtype))


# ---- frequency embedding ------------------------------------------------------------------------------------------------------------
def freq_cols(D, n_freq):
    return D + 2 * D * n_freq


def freq_forward(x, n_freq, dtype=np.float64):
    """y [B, C]: x, then per frequency f the D columns sin(2^f x) and the D columns sin(2^f x + pi/2).  float32: the argument is formed
    in fp32 as the kernels do (exact scaling, one rounded add of the fp32 pi/2); float64: sin of the exact argument 2^f x + k pi/2"""
    x = np.asarray(x).astype(dtype)
    parts = [x]
    for f in range(n_freq):
        a = x * dtype(2.0 ** f)
        parts += [np.sin(a), np.sin(a + dtype(np.pi / 2))]
    return np.concatenate(parts, axis=1)


def _split(t, D, n_freq):
    """[B, C] -> (identity block [B, D], k = 0 blocks [B, n, D], k = 1 blocks [B, n, D])"""
    r = t[:, D:].reshape(t.shape[0], n_freq, 2, D)
    return t[:, :D], r[:, :, 0], r[:, :, 1]


def freq_backward(g, y, D, n_freq, dtype=np.float64, absolute=False):
    """gx [B, D] = g_d + sum_f 2^f (g_f0 y_f1 - g_f1 y_f0) from the forward's OUTPUTS y; absolute: the sum of the absolute terms"""
    g, y = np.asarray(g).astype(dtype), np.asarray(y).astype(dtype)
    g_id, g0, g1 = _split(g, D, n_freq)
    _, y0, y1 = _split(y, D, n_freq)
    s = (2.0 ** np.arange(n_freq)).astype(dtype)[None, :, None]
    if absolute:
        return np.abs(g_id) + (s * (np.abs(g0 * y1) + np.abs(g1 * y0))).sum(1)
    return g_id + (s * (g0 * y1 - g1 * y0)).sum(1)


def freq_backward_backward(v, g, y, D, n_freq, dtype=np.float64, absolute=False):
    """(dL/dg [B, C], dL/dx [B, D]) for v = dL/d(gx); absolute: the sums of absolute terms behind each"""
    v, g, y = (np.asarray(t).astype(dtype) for t in (v, g, y))
    _, g0, g1 = _split(g, D, n_freq)
    _, y0, y1 = _split(y, D, n_freq)
    s = (2.0 ** np.arange(n_freq)).astype(dtype)[None, :, None]
    vv = v[:, None, :]
    d0, d1 = vv * s * y1, -vv * s * y0
    dg = np.concatenate([v, np.stack([d0, d1], 2).reshape(v.shape[0], 2 * n_freq * D)], axis=1)
    if absolute:
        return np.abs(dg), np.abs(v) * (s * s * (np.abs(g0 * y0) + np.abs(g1 * y1))).sum(1)
    return dg, -v * (s * s * (g0 * y0 + g1 * y1)).sum(1)


def ulp32(a):
    """spacing of float32 at |a| (a float64 array)"""
    return np.spacing(np.abs(np.asarray(a, np.float64)).astype(np.float32)).astype(np.float64)


def freq_arg_term(x, n_freq):
    """[B, C]: half an ulp of float32 at |2^f x_d| + pi/2 for the sine columns, 0 for the identity columns: what forming the argument
    in fp32 costs a |sin'| <= 1 function"""
    x = np.asarray(x).astype(np.float64)
    parts = [np.zeros_like(x)]
    for f in range(n_freq):
        t = 0.5 * ulp32(np.abs(x) * 2.0 ** f + np.pi / 2)
        parts += [t, t]
    return np.concatenate(parts, axis=1)


# ---- tolerances of the frequency embedding (derived; used by the CPU and the GPU tests) ----------------------------------------------
EPS = 2.0 ** -24


def freq_value_tol(x, n_freq, c):
    """|y - sin64(2^f x + k pi/2)| <= 1/2 ulp32(|2^f x| + pi/2) + c 2^-24 (identity columns: 0): the fp32 argument, then c units for
    the sine itself and the rounded pi/2"""
    t = freq_arg_term(x, n_freq)
    return np.where(t > 0, t + c * EPS, 0.0)


def freq_grad_tol(x, g, n_freq, c, y_exact):
    """bound of |gx - gx64| [B, D] when gx is formed in fp32 from outputs that carry the error of freq_value_tol: the error of every y
    enters through its own term (2^f |g| dy), plus (2 n_freq + 2) roundings on the sum of the absolute terms"""
    D = np.asarray(x).shape[1]
    g = np.asarray(g, np.float64)
    dy = freq_value_tol(x, n_freq, c)
    _, g0, g1 = _split(g, D, n_freq)
    _, e0, e1 = _split(dy, D, n_freq)
    s = (2.0 ** np.arange(n_freq))[None, :, None]
    prop = (s * (np.abs(g0) * e1 + np.abs(g1) * e0)).sum(1)
    return prop + (2 * n_freq + 2) * EPS * freq_backward(g, y_exact, D, n_freq, absolute=True)


def eikonal_program(x, g, n_freq):
    """fp64: y, n = gx, L = mean((|n| - 1)^2), v = dL/dn, and (dL/dg, dL/dx) through the double backward"""
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    B, D = x.shape
    y = freq_forward(x, n_freq)
    n = freq_backward(g, y, D, n_freq)
    nn = np.linalg.norm(n, axis=1, keepdims=True)
    v = 2.0 / B * (nn - 1.0) * n / nn
    dg, dx = freq_backward_backward(v, g, y, D, n_freq)
    return dict(y=y, n=n, norm=nn, v=v, dg=dg, dx=dx)


def eikonal_tols(x, g, n_freq, c):
    """bounds of |g.grad - dg64| [B, C] and |x.grad - dx64| [B, D] for the fp32 program  y -> n -> v = dL/dn -> double backward:
    dn = freq_grad_tol;  v = (2/B)(1 - 1/|n|) n, so |dv_d| <= (2/B)(|1 - 1/|n|| dn_d + |n_d| / |n|^3 sum_e |n_e| dn_e) plus 8 roundings
    of its own fp32 evaluation (norm, subtraction, division, scaling);  the outputs are products v 2^f y and v 4^f g y: each factor's
    error times the absolute value of the others, plus (2 n_freq + 2) roundings on the sum of the absolute terms."""
    P = eikonal_program(x, g, n_freq)
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    B, D = x.shape
    y, n, nn, v = P["y"], P["n"], P["norm"], P["v"]
    dn = freq_grad_tol(x, g, n_freq, c, y)
    dv = 2.0 / B * (np.abs(1 - 1 / nn) * dn + np.abs(n) / nn ** 3 * (np.abs(n) * dn).sum(1, keepdims=True))
    dv = dv + 8 * EPS * 2.0 / B * np.abs(n) * (1 + 1 / nn)
    dy = freq_value_tol(x, n_freq, c)
    _, g0, g1 = _split(g, D, n_freq)
    _, y0, y1 = _split(y, D, n_freq)
    _, e0, e1 = _split(dy, D, n_freq)
    s = (2.0 ** np.arange(n_freq))[None, :, None]
    av, adv = np.abs(v)[:, None, :], dv[:, None, :]
    t0 = adv * s * np.abs(y1) + av * s * e1
    t1 = adv * s * np.abs(y0) + av * s * e0
    abs_dg, abs_dx = freq_backward_backward(v, g, y, D, n_freq, absolute=True)
    tol_dg = np.concatenate([dv, np.stack([t0, t1], 2).reshape(B, 2 * n_freq * D)], axis=1) + (2 * n_freq + 2) * EPS * abs_dg
    sum_abs = (s * s * (np.abs(g0 * y0) + np.abs(g1 * y1))).sum(1)
    tol_dx = dv * sum_abs + np.abs(v) * (s * s * (np.abs(g0) * e0 + np.abs(g1) * e1)).sum(1) + (2 * n_freq + 2) * EPS * abs_dx
    return tol_dg, tol_dx
