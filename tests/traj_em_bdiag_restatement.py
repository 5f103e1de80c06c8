"""numpy restatement of EM re-estimation over all mixtures for a trajectory converter made straight from a CROSS-DIAGONAL model
(BlockDiagTrajectoryEMGMMMap, vcmi_traj_set_em_bdiag, csrc/traj_em_bdiag.hip) -- test infrastructure, written from the
cross-diagonal parameters alone (no (4D,4D,M) tensor, no inverse) and sharing no code with the product.

Notation of tests/traj_bdiag_restatement.py.  Per mixture m and feature k = 0 .. 2D-1 =: K-1, source side x, target side y:
    l_tm   centred source log-density (gmmmap_bdiag_restatement.logdens; -inf for w_m <= 0)
    a = c / vx,  q = 1 / (vy - a c),  E_kmt = muy_km + a_km (x_kt - mux_km),  c_m = 1/2 sum_k log q_km
    Y_t(y) = (W y)_t = [y_t ; (y_{t+1} - y_{t-1}) / 2], a missing neighbour dropped (T = 1: zero deltas)
E-step at y:   l'_mt = (l_tm - lse_m l_tm) + c_m - 1/2 sum_k q_km (Y_kt - E_kmt)^2 - D log 2 pi
               lse_t = logsumexp_m l'_mt,  gamma_mt = exp(l'_mt - lse_t),  L(y) = sum_t lse_t
M-step:        qbar_kt = sum_m gamma_mt q_km,  gbar_kt = sum_m gamma_mt q_km E_kmt, then per static dimension and frame parity
               P[t,t] = p_s(t) + p_d(t-1)/4 + p_d(t+1)/4,  P[t,t-2] = -p_d(t-1)/4,  r[t] = g_s(t) + g_d(t-1)/2 - g_d(t+1)/2
               with (p, g) = (qbar, gbar), assembled and solved densely
y^0 is traj_bdiag_restatement.BdiagTrajectory.tridiag (arg-max); iteration j maps y^j to y^{j+1}.

BOUNDS (eps = 2^-53; starred quantities exact, here: evaluated in longdouble; every bound is a function of the inputs and of the
longdouble evaluation, none of a result under test).

 (1) l'_mt.  B_mt = Bs_mt + Bx_t + Bt_mt + Bc_m + 2 eps (|l - lse_m l| + |c_m - D log 2pi - tq| + |l'|) with
     Bs  gmmmap_bdiag_restatement.logdens_bound (the source term: (K + 16) eps of its absolute terms);
     Bx  of lse_m l: max_m Bs_mt + (M + 16) eps (1 + |lse_m l|) -- logsumexp moves by at most the largest shift of its arguments,
         the sum of M exponentials, the logarithm and the final sum are the second term;
     Bt  of tq = 1/2 sum_k q e^2, e = Y - E.  Y's delta rows carry one rounding (eps |Y|); E as the kernel forms it 3 eps (|muy| +
         |a dx|) (gmmmap_bdiag_restatement: the difference, the quotient a, the fma); the difference one more: |de| <= eps (|Y| + 3
         (|muy| + |a dx|) + |e|) -- an ABSOLUTE bound in the size of the operands, so the cancellation in Y - E is inside it.
         Then d(q e^2) <= q (2 |e| de + de^2) + 5 eps q e^2 (q's three roundings, the square, the product) and K chained fmas:
         Bt = 1/2 sum_k q (2 |e| de + de^2) + 1/2 (K + 8) eps sum_k q e^2;
     Bc  of c_m - D log 2pi: (K + 16) eps (1/2 sum_k |log q| + D log 2pi) + 3/2 K eps (log of a q with relative error 3 eps).
 (2) lse_t.  logsumexp(l' + d) - logsumexp(l') = log sum_m gamma*_m exp(d_m), so with |d_m| <= B_m
         BL_t = log1p(sum_m gamma*_mt expm1(B_mt)) + (M + 16) eps (1 + |lse_t|)
     (the lower side, -log sum gamma exp(-B), is no larger); a far mixture's large B is weighted by its small gamma.
 (3) gamma_mt = exp(l' - lse) (or exp(l' - u) / sum: the same to these terms) has RELATIVE error
         G_mt = expm1(B_mt + BL_t + 2 eps |l'_mt - lse_t| + (M + 16) eps),   dgamma = gamma* G
     and element-wise
         |d qbar_kt| <= sum_m dgamma_mt q_km + (M + 4) eps sum_m gamma* q
         |d gbar_kt| <= sum_m dgamma_mt q_km (|muy| + |a dx|) + (M + 12) eps sum_m gamma* q (|muy| + |a dx|)
     in the style of posterior_bound / convert_bound (q's three roundings, E's three, the products and the M chained fmas).
 (4) one E/M pair from the SAME y^j: relerr(y^{j+1}) <= 64 cond rho eps + cond_inf (dP + dr), cond / rho of the blended systems as
     traj_bdiag_restatement reports them for the arg-max ones (cond in the 2-norm: traj_diag_restatement.tolerance), cond_inf the
     largest infinity-norm condition number, and per static dimension dP = max_t (dq_s(t) + dq_d(t-1)/2 + dq_d(t+1)/2) / max_t
     P[t,t] (row sums of the perturbation of P over the largest row of P), dr = max_t (dg_s(t) + dg_d(t-1)/2 + dg_d(t+1)/2) /
     max_t |r[t]| with (dq, dg) the bounds of (3); the largest dP + dr over the static dimensions is taken.  (A system of
     condition number c turns relative perturbations dP, dr into at most c (dP + dr) of the solution, to first order.)
 (5) k pairs end to end: s_0 = 64 cond rho eps of the arg-max solve, s_{j+1} = (4) at y^j, kappa_j = the amplification of pair j
     (below); bound_k = sum_{j <= k} s_j prod_{j <= i < k} kappa_i.  kappa_j is MEASURED on the restatement: a perturbation of
     1e-8 ||y^j|| in 8 seeded random (Gaussian) directions through one restated pair, the largest ||change of y^{j+1}|| /
     ||y^{j+1}|| over 1e-8 in the Euclidean norm -- the norm in which the E/M map contracts -- doubled (random directions
     underestimate the worst), floored at 1.  Undoubled it is 0.03 .. 0.50 for the cases below (tests/test_traj_em_bdiag_host.py
     asserts doubled <= 2), so bound_k is the plain sum of the single-step bounds.
 (6) the objective: |L(y) - L*(y)| <= sum_t BL_t at the same y; at trajectories that differ by at most D_j = bound_j max |y^j|
     element-wise, dL/dY_kt = gbar_kt - qbar_kt Y_kt and every |dY| <= D_j, so
         |L_j - L*_j| <= sum_t BL_t + 2 D_j sum_kt |gbar_kt - qbar_kt Y_kt|           (2: the second-order remainder)."""
import functools

import numpy as np

import gmmmap_bdiag_restatement as BR
import traj_bdiag_restatement as R
import traj_diag_restatement as DR

LD = np.longdouble
EPS = 2.0 ** -53
NITER = 4

TILE_CASE = (12, 4, [63, 64, 65, 129, 1])
# name -> (D, M, Ts, index of a zeroed weight or None)
CASES = {f"{D}-{M}": (D, M, tuple(Ts), None) for D, M, Ts in R.SHAPES}
CASES["tiles-12-4"] = (TILE_CASE[0], TILE_CASE[1], tuple(TILE_CASE[2]), None)
CASES["zero-weight-12-4"] = (TILE_CASE[0], TILE_CASE[1], tuple(TILE_CASE[2]), 2)
CASES["vc-12-4"] = (R.VC_CASE[0], R.VC_CASE[1], tuple(R.VC_CASE[2]), None)
# ... and where the kernel's own launch rule (csrc/traj_em_bdiag_plan.hpp) takes its 32-frame tiles, which none of the shapes above
# does: the largest feature dimension with one round of mixtures, and four rounds of mixtures at a small one
CASES["small-tile-64-56"] = (64, 56, (33, 70), None)
CASES["small-tile-20-240"] = (20, 240, (70, 31), None)
# the cases the dense restatement (traj_em_restatement.em_convert on the expanded model) is compared on
DENSE_CASES = [k for k, v in CASES.items() if v[0] <= 40 and v[1] <= 8]


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """-> (w, mu, covars), [X (T, 2D) per utterance]; never written to"""
    D, M, Ts, zero = CASES[name]
    (w, mu, cov), Xs = R.make_case(D, M, list(Ts))
    if zero is not None:
        w = np.array(w, dtype=np.float64)
        w[zero] = 0.0
        w /= w.sum()
    return (w, mu, cov), Xs


class Model:
    """the per-model constants in `dtype`"""

    def __init__(self, w, mu, covars, swap=False, dtype=np.float64):
        self.args = (w, mu, covars, swap)
        self.dtype = dtype
        self.w, self.mux, self.muy, vx, self.a = BR.split(w, mu, covars, swap, dtype)
        cov = np.asarray(covars, dtype=dtype)
        K = cov.shape[0] // 3
        vy, c = (cov[:K] if swap else cov[K:2 * K]), cov[2 * K:]
        self.q = 1 / (vy - self.a * c)                                    # (K, M)
        self.K, self.D, self.M = K, K // 2, cov.shape[1]
        self.log2pi = np.log(2 * np.arccos(dtype(-1)))
        self.c = np.log(self.q).sum(axis=0) / 2                           # (M,)

    def stencil(self, y):
        """y (T, D) -> Y (T, 2D)"""
        y = np.asarray(y, dtype=self.dtype)
        T, D = y.shape
        Y = np.zeros((T, 2 * D), dtype=self.dtype)
        Y[:, :D] = y
        Y[:-1, D:] += y[1:] / 2
        Y[1:, D:] -= y[:-1] / 2
        return Y

    def estep(self, X, y, reverse=False):
        """-> dict: ell (T,M), lse (T), gamma (T,M), L, qbar (T,K), gbar (T,K), and the pieces the bounds need.  reverse: the
        sums over k and over m taken in descending order (a second operation order of the same statement)"""
        X = np.asarray(X, dtype=self.dtype)
        T, M = X.shape[0], self.M
        o = slice(None, None, -1) if reverse else slice(None)
        Ls = BR.logdens(X, *self.args, self.dtype)                        # (T, M)
        with np.errstate(invalid="ignore"):
            us = Ls.max(axis=1)
            lsx = us + np.log(np.exp(Ls - us[:, None])[:, o].sum(axis=1))
        Y = self.stencil(y)
        ell = np.full((T, M), -np.inf, dtype=self.dtype)
        tq = np.zeros((T, M), dtype=self.dtype)
        E = np.zeros((M, T, self.K), dtype=self.dtype)
        for m in range(M):
            E[m] = self.muy[:, m] + self.a[:, m] * (X - self.mux[:, m])
            e = Y - E[m]
            tq[:, m] = (self.q[:, m] * e * e)[:, o].sum(axis=1) / 2
            if self.w[m] > 0:
                ell[:, m] = (Ls[:, m] - lsx) + ((self.c[m] - self.D * self.log2pi) - tq[:, m])
        u = ell.max(axis=1)
        lse = u + np.log(np.exp(ell - u[:, None])[:, o].sum(axis=1))
        gamma = np.exp(ell - lse[:, None])
        qbar, gbar = np.zeros_like(X), np.zeros_like(X)
        for m in (range(M - 1, -1, -1) if reverse else range(M)):
            qbar += gamma[:, m:m + 1] * self.q[:, m]
            gbar += gamma[:, m:m + 1] * self.q[:, m] * E[m]
        return dict(ell=ell, lse=lse, gamma=gamma, L=lse.sum(), qbar=qbar, gbar=gbar, Ls=Ls, lsx=lsx, tq=tq, E=E, Y=Y)


def solve(p, g, dp=None, dg=None, ga=None, conds=True):
    """the tridiagonal systems of (p, g) (T, 2D), float64 -> dict: y (T, D); cond (2-norm), cond_inf: the largest over the systems;
    rho = max r_abs / max |r| with r_abs the stencil over ga (all signs positive; ga None: |g|); with (dp, dg) element-wise bounds
    of (p, g): prop = the largest dP + dr of bound (4) over the static dimensions.  conds=False: y alone (cond = cond_inf = 1)"""
    p, g = np.asarray(p, dtype=np.float64), np.asarray(g, dtype=np.float64)
    T, D = p.shape[0], p.shape[1] // 2
    y = np.zeros((T, D))
    if T == 0:
        return dict(y=y, cond=1.0, cond_inf=1.0, rho=1.0, prop=0.0)

    def st(a, sign):                        # the stencil over (T, 2D) -> (T, D): a_s(t) + a_d(t-1)/2 + sign a_d(t+1)/2
        out = a[:, :D].copy()
        out[1:] += 0.5 * a[:-1, D:]
        out[:-1] += sign * 0.5 * a[1:, D:]
        return out

    ps, pd = p[:, :D], p[:, D:]
    diag = ps.copy()
    diag[1:] += 0.25 * pd[:-1]
    diag[:-1] += 0.25 * pd[1:]
    r = st(g, -1.0)
    ra = st(np.abs(g) if ga is None else np.asarray(ga, dtype=np.float64), 1.0)
    cond = cond_inf = 1.0
    for par in (0, 1):
        fr = np.arange(par, T, 2)
        K = len(fr)
        if K == 0:
            continue
        P = np.zeros((D, K, K))
        k = np.arange(K)
        P[:, k, k] = diag[fr].T
        if K > 1:
            e = -0.25 * pd[fr[1:] - 1].T
            P[:, k[1:], k[:-1]] = e
            P[:, k[:-1], k[1:]] = e
        y[fr] = np.linalg.solve(P, r[fr].T[:, :, None])[:, :, 0].T
        if conds:
            cond = max(cond, float(np.max(np.linalg.cond(P))))
            cond_inf = max(cond_inf, float(np.max(np.linalg.cond(P, np.inf))))
    prop = 0.0
    if dp is not None:
        dP = st(np.asarray(dp, dtype=np.float64), 1.0).max(axis=0) / diag.max(axis=0)
        dr = st(np.asarray(dg, dtype=np.float64), 1.0).max(axis=0) / np.abs(r).max(axis=0)
        prop = float(np.max(dP + dr))
    return dict(y=y, cond=cond, cond_inf=cond_inf, rho=float(np.max(ra) / np.max(np.abs(r))), prop=prop)


def estep_bounds(model, X, y):
    """bounds (1)-(3) at y from the longdouble evaluation -> dict of float64: ell (T,M; inf for w_m <= 0), lse (T), qbar (T,K), gbar
    (T,K), gabs (T,K) = sum_m gamma* q (|muy| + |a dx|), and the longdouble E-step `ref`"""
    w, mu, cov, swap = model
    md = Model(w, mu, cov, swap, LD)
    X = np.asarray(X, dtype=LD)
    ref = md.estep(X, y)
    T, K, M = X.shape[0], md.K, md.M
    Bs = BR.logdens_bound(X, w, mu, cov, swap)                                       # inf where w_m <= 0
    live = np.asarray(md.w > 0)
    Bx = np.where(np.isfinite(Bs), Bs, 0.0).max(axis=1) + (M + 16) * EPS * (1 + np.abs(ref["lsx"]))
    Y, Yabs = ref["Y"], np.abs(ref["Y"])
    B = np.full((T, M), np.inf, dtype=LD)
    Eabs = np.zeros((M, T, K), dtype=LD)
    for m in range(M):
        adx = md.a[:, m] * (X - md.mux[:, m])
        Eabs[m] = np.abs(md.muy[:, m]) + np.abs(adx)
        if not live[m]:
            continue
        e = np.abs(Y - ref["E"][m])
        de = EPS * (Yabs + 3 * Eabs[m] + e)
        q = md.q[:, m]
        Bt = (q * (2 * e * de + de * de)).sum(axis=1) / 2 + (K + 8) * EPS * ref["tq"][:, m]
        Bc = (K + 16) * EPS * (np.abs(np.log(q)).sum() / 2 + md.D * md.log2pi) + 1.5 * K * EPS
        lp, ct = ref["Ls"][:, m] - ref["lsx"], (md.c[m] - md.D * md.log2pi) - ref["tq"][:, m]
        B[:, m] = Bs[:, m] + Bx + Bt + Bc + 2 * EPS * (np.abs(lp) + np.abs(ct) + np.abs(ref["ell"][:, m]))
    gam = ref["gamma"]
    Bl = np.where(live[None, :], B, 0.0)
    BL = np.log1p((gam * np.expm1(Bl)).sum(axis=1)) + (M + 16) * EPS * (1 + np.abs(ref["lse"]))
    with np.errstate(invalid="ignore"):
        dist = np.where(live[None, :], np.abs(ref["ell"] - ref["lse"][:, None]), 0.0)
    dgam = gam * np.expm1(Bl + BL[:, None] + 2 * EPS * dist + (M + 16) * EPS)
    dq, dg, sq, gabs = (np.zeros((T, K), dtype=LD) for _ in range(4))
    for m in range(M):
        q = md.q[:, m]
        dq += dgam[:, m:m + 1] * q
        dg += dgam[:, m:m + 1] * q * Eabs[m]
        sq += gam[:, m:m + 1] * q
        gabs += gam[:, m:m + 1] * q * Eabs[m]
    f64 = lambda a: np.asarray(a, dtype=np.float64)                                   # noqa: E731
    return dict(ell=f64(B), lse=f64(BL), qbar=f64(dq + (M + 4) * EPS * sq), gbar=f64(dg + (M + 12) * EPS * gabs), gabs=f64(gabs),
                ref=ref)


def one_pair(model, X, y):
    """one restated E/M pair from y (float64 arithmetic) -> dict: y (T,D) the next trajectory, L = L(y given), step = bound (4),
    BL = sum_t BL_t, grad = sum_kt |gbar - qbar Y|, est = the float64 E-step"""
    w, mu, cov, swap = model
    est = Model(w, mu, cov, swap).estep(X, y)
    b = estep_bounds(model, X, y)
    s = solve(est["qbar"], est["gbar"], b["qbar"], b["gbar"], b["gabs"])
    step = DR.tolerance(s["cond"]) * s["rho"] + s["cond_inf"] * s["prop"]
    grad = float(np.abs(est["gbar"] - est["qbar"] * est["Y"]).sum())
    return dict(y=s["y"], L=float(est["L"]), step=step, BL=float(b["lse"].sum()), grad=grad, est=est, cond=s["cond"], rho=s["rho"])


def kappa(model, X, y, ynext, ndir=8, rel=1e-8):
    """amplification of one pair at y (bound (5)), in the Euclidean norm: -> (doubled and floored, undoubled)"""
    w, mu, cov, swap = model
    md = Model(w, mu, cov, swap)
    rng = np.random.default_rng(12345)
    scale, out = float(np.linalg.norm(y)), float(np.linalg.norm(ynext))
    worst = 0.0
    for _ in range(ndir):
        d = rng.standard_normal(y.shape)
        d *= rel * scale / np.linalg.norm(d)
        e = md.estep(X, y + d)
        y2 = solve(e["qbar"], e["gbar"], conds=False)["y"]
        worst = max(worst, float(np.linalg.norm(y2 - ynext)) / out / rel)
    return max(1.0, 2.0 * worst), worst


def em_convert(model, X, n=NITER):
    """X (T, 2D) -> dict: ys [n+1] of (T,D); L [n+1] (entry j = L(y^j)); bound [n+1]: bound (5) of y^j; Lbound [n+1]: bound (6) of
    L_j; step [n+1]: s_j; kappa [n]: (doubled, undoubled) of pair j; gamma0: gamma at y^0"""
    w, mu, cov, swap = model
    X = np.asarray(X, dtype=np.float64)
    y, cond, rho = R.BdiagTrajectory(w, mu, cov, swap).tridiag(X)
    out = dict(ys=[y], L=[], bound=[DR.tolerance(cond) * rho], Lbound=[], step=[DR.tolerance(cond) * rho], kappa=[], gamma0=None)
    for j in range(n + 1):
        pr = one_pair(model, X, out["ys"][j])
        if j == 0:
            out["gamma0"] = pr["est"]["gamma"]
        out["L"].append(pr["L"])
        out["Lbound"].append(pr["BL"] + 2.0 * out["bound"][j] * float(np.max(np.abs(out["ys"][j]))) * pr["grad"])
        if j == n:
            break
        kap = kappa(model, X, out["ys"][j], pr["y"])
        out["ys"].append(pr["y"])
        out["step"].append(pr["step"])
        out["kappa"].append(kap)
        out["bound"].append(out["bound"][j] * kap[0] + pr["step"])
    return out


@functools.lru_cache(maxsize=None)
def case_reference(name, n=NITER):
    """em_convert of every non-empty utterance of the case, computed once and never written to"""
    (w, mu, cov), Xs = case_inputs(name)
    return [em_convert((w, mu, cov, False), X, n) for X in Xs]
