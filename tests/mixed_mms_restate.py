"""solver/mixed_cg_mms_tm_nd.c:69-511 restated in NumPy, statement by statement: the yardstick of the device solver on shapes that
have no run of the reference.  No GPU or torch dependency.

Fields of the loop are complex64 [N][4][3] (oracle/nd_restate.py's layout in single precision), the solutions P and the fields of a
reliable update complex128.  Scalars are Python floats (doubles) and are rounded with np.float32 exactly where the reference casts
them or hands them to a `float` parameter; square_norm_32 and scalar_prod_r_32 accumulate in double and return a float per flavour.
f32(u, d) -> (Au, Ad) is the fp32 operator on complex64 pairs, f64 the fp64 one on complex128 pairs.
"""
import numpy as np

F = np.float32


def _nsq32(a):
    """square_norm_32: double accumulation, float return"""
    a = a.astype(np.complex128)
    return float(F((a.real ** 2).sum() + (a.imag ** 2).sum()))


def _dot32(a, b):
    """scalar_prod_r_32: double accumulation, float return"""
    a, b = a.astype(np.complex128), b.astype(np.complex128)
    return float(F((a.real * b.real).sum() + (a.imag * b.imag).sum()))


def _nsq64(a):
    return float((a.real ** 2).sum() + (a.imag ** 2).sum())


def rounded_op(f64):
    """An fp32 operator from an fp64 one: the input is widened, the output rounded to float32 once per application."""
    def f32(u, d):
        au, ad = f64(u.astype(np.complex128), d.astype(np.complex128))
        return au.astype(np.complex64), ad.astype(np.complex64)
    return f32


def mixed_cg_mms_tm_nd(f64, f32, Q_up, Q_dn, shifts, max_iter, eps_sq, rel_prec, fallback=None):
    """Returns (return value, [(P_up, P_dn) per shift] as complex128, info); info: "updates" = [[iteration, trigger shift], ..],
    "removals" = [[iteration, shifts remaining], ..], "active", "fallback".  fallback(Q_up, Q_dn) -> (ret, P) serves |Q|^2 < 1e-4."""
    noshifts = len(shifts)
    info = {"updates": [], "removals": [], "fallback": False, "active": noshifts}
    rr = _nsq64(Q_up) + _nsq64(Q_dn)                                              # :105-107
    if rr < 1.0e-4:                                                               # :110-113
        info["fallback"] = True
        ret, P = fallback(Q_up, Q_dn)
        return ret, P, info
    r0r0 = rr_old = rr
    c64 = np.complex64
    P = [[np.zeros_like(Q_up, dtype=np.complex128), np.zeros_like(Q_dn, dtype=np.complex128)] for _ in range(noshifts)]   # :264-267
    x = [[np.zeros(Q_up.shape, c64), np.zeros(Q_up.shape, c64)] for _ in range(noshifts)]
    d = [[Q_up.astype(c64), Q_dn.astype(c64)] for _ in range(noshifts)]          # :231-232, :255-256
    r = [Q_up.astype(c64), Q_dn.astype(c64)]                                      # :227-228
    x_d = [np.zeros_like(P[0][0]), np.zeros_like(P[0][1])]
    sigma = [shifts[0] * shifts[0]] + [shifts[im] * shifts[im] - shifts[0] * shifts[0] for im in range(1, noshifts)]
    zitam1, zita = [0.0] + [1.0] * (noshifts - 1), [0.0] + [1.0] * (noshifts - 1)   # [0]: calloc, never written
    alphas, betas = [1.0] * noshifts, [0.0] * noshifts
    res, res0, maxres = [rr] * noshifts, [rr] * noshifts, [rr] * noshifts
    rel_delta, trigger_shift = 1.0e-10, -1
    j = 0
    for j in range(max_iter + 1):
        if j == max_iter:
            break
        Ad = list(f32(d[0][0], d[0][1]))                                          # :276
        Ad[0] = Ad[0] + F(sigma[0]) * d[0][0]                                     # :278-279
        Ad[1] = Ad[1] + F(sigma[0]) * d[0][1]
        dAd = _dot32(d[0][0], Ad[0]) + _dot32(d[0][1], Ad[1])                     # :283-286
        alpham1 = alphas[0]
        alphas[0] = rr_old / dAd
        r[0] = r[0] + F(-alphas[0]) * Ad[0]                                       # :292-293
        r[1] = r[1] + F(-alphas[0]) * Ad[1]
        rr = _nsq32(r[0]) + _nsq32(r[1])                                          # :296-298
        if (rel_prec == 0 and rr <= eps_sq) or (rel_prec != 0 and rr <= eps_sq * r0r0):   # :307
            break
        for im in range(1, noshifts):                                             # :317-323
            gamma = zita[im] * alpham1 / (alphas[0] * betas[0] * (1. - zita[im] / zitam1[im]) + alpham1 * (1. + sigma[im] * alphas[0]))
            zitam1[im] = zita[im]
            zita[im] = gamma
            alphas[im] = alphas[0] * zita[im] / zitam1[im]
        res[0] = rr                                                               # :326-334
        for im in range(1, noshifts):
            res[im] = rr * zita[im]
        rel_update = False
        for im in range(noshifts - 1, -1, -1):
            if res[im] > maxres[im]:
                maxres[im] = res[im]
            if res[im] < rel_delta * res0[im] and res0[im] <= maxres[im]:
                rel_update = True
            if rel_update and trigger_shift == -1:
                trigger_shift = im
        for im in range(noshifts):                                                # :340-347 / :370-377
            x[im][0] = x[im][0] + F(alphas[im]) * d[im][0]
            x[im][1] = x[im][1] + F(alphas[im]) * d[im][1]
        if not rel_update:
            betas[0] = rr / rr_old                                                # :350-351
            rr_old = rr
        else:
            info["updates"].append([j, trigger_shift])
            for im in range(noshifts):                                            # :373-380
                P[im][0] += x[im][0]
                P[im][1] += x[im][1]
            x_d[0] += x[0][0]                                                     # :383-384
            x_d[1] += x[0][1]
            Ax = f64(x_d[0], x_d[1])                                              # :387-397
            r_d = [Q_up - (Ax[0] + sigma[0] * x_d[0]), Q_dn - (Ax[1] + sigma[0] * x_d[1])]
            rr = _nsq64(r_d[0]) + _nsq64(r_d[1])
            res[0] = rr
            if res[trigger_shift] > res0[trigger_shift] and trigger_shift == 0:   # :404-408
                break
            for im in range(noshifts):                                            # :411-416
                x[im][0][...] = 0
                x[im][1][...] = 0
            r = [r_d[0].astype(c64), r_d[1].astype(c64)]                          # :419-420
            betas[0] = res[0] / rr_old                                            # :424-425
            rr_old = rr
        d[0][0] = F(betas[0]) * d[0][0] + r[0]                                    # :354-355 / :427-428
        d[0][1] = F(betas[0]) * d[0][1] + r[1]
        for im in range(1, noshifts):                                             # :358-362 / :430-434
            betas[im] = betas[0] * zita[im] * alphas[im] / (zitam1[im] * alphas[0])
            d[im][0] = F(betas[im]) * d[im][0] + F(zita[im]) * r[0]
            d[im][1] = F(betas[im]) * d[im][1] + F(zita[im]) * r[1]
        if rel_update:                                                            # :437-441
            res[trigger_shift] = res[0] * zita[trigger_shift] * zita[trigger_shift]
            res0[trigger_shift] = maxres[trigger_shift] = res[trigger_shift]
            trigger_shift = -1
        if j > 0 and j % 10 == 0 and noshifts > 1:                                # :445-459: the last active shift, on the updated d
            im = noshifts - 1
            sn = _nsq32(d[im][0]) + _nsq32(d[im][1])
            if alphas[im] * alphas[im] * sn <= eps_sq:
                noshifts -= 1
                info["removals"].append([j, noshifts])
                P[im][0] += x[im][0]
                P[im][1] += x[im][1]
    for im in range(noshifts):                                                    # :466-475
        P[im][0] += x[im][0]
        P[im][1] += x[im][1]
    info["active"] = noshifts
    return (j if j < max_iter else -1), [tuple(p) for p in P], info


# ---------------------------------------------------------------- what the tests of the solver share: inputs and yardsticks
def count_rule(it, ref):
    """the rule of tests/test_gpu_nd32.py"""
    return abs(it - ref) <= max(3, ref // 8)


def distance(P, X):
    """sqrt(|P - X|^2 / |X|^2) over both flavours of a pair, the `distance_to_cg_mms_tm_nd` of the fixtures"""
    num = sum(float((np.abs(np.asarray(p) - np.asarray(x)) ** 2).sum()) for p, x in zip(P, X))
    den = sum(float((np.abs(np.asarray(x)) ** 2).sum()) for x in X)
    return float(np.sqrt(num / den))


def operators(orc, mubar, epsbar, invmaxev):
    """(f64, f32) on the CPU oracle's Hopping_Matrix: Qtm_pm_ndpsi of oracle/nd_restate.py and its image rounded to float32"""
    from oracle import nd_restate as nd
    H = nd.hop_over(orc.Hopping_Matrix, orc.Vh)

    def f64(u, d):
        return nd.Qtm_pm_ndpsi(H, u, d, mubar, epsbar, invmaxev)
    return f64, rounded_op(f64)


def restate_run(f64, f32, qu, qd, shifts, run, max_iter):
    """One run of the fixtures' parameter sets (`run`: an entry of ref_mixed_mms_scalars_*.json["runs"]) through the restatement, and
    the fp64 multi-shift solve it is measured against: (ret, P, info, X)."""
    from oracle import nd_restate as nd
    sh = shifts[:run["nshifts"]]
    qu, qd = run["source_scale"] * qu, run["source_scale"] * qd

    def fb(a, b):
        ret, P, _, _ = nd.cg_mms_tm_nd(f64, a, b, sh, max_iter, run["eps_sq"], run["rel_prec"])
        return ret, P
    ret, P, info = mixed_cg_mms_tm_nd(f64, f32, qu, qd, sh, max_iter, run["eps_sq"], run["rel_prec"], fallback=fb)
    _, X, _, _ = nd.cg_mms_tm_nd(f64, qu, qd, sh, max_iter, 1e-22, 0)
    return ret, P, info, X
