"""Scenes for the tests of lf_mkd_bundle_adjust_intrinsics_device, and a plain float64 numpy restatement of its algorithm
(include/lf_mkd.h): tests/bundle_cases.py's Levenberg-Marquardt loop with the shared intrinsics of the groups beside the
cameras and the points -- the group rows, the three extra blocks, the block-Jacobi preconditioned conjugate gradients over
cameras and groups with the same stopping rules -- written with numpy's own sums and solves.  It shares no code with
csrc/mkd_bundle_math.h; tests/test_bundle_intr_twin.py holds the host twin to it.

A scene is tests/bundle_cases.py's dict with `camera_group` (uint32 [n_images] or None) and `n_groups`."""
import numpy as np

import bundle_cases as cases


def with_groups(s, camera_group=None, n_groups=1, scale=1.0, shift=(0.0, 0.0)):
    """the scene with a group map, its input focal lengths times `scale` and its principal points moved by `shift`"""
    K = np.asarray(s["intrinsics"], np.float32).copy()
    K[:, :2] *= np.float32(scale)
    K[:, 2] += np.float32(shift[0])
    K[:, 3] += np.float32(shift[1])
    g = None if camera_group is None else np.asarray(camera_group, np.uint32).copy()
    return dict(s, intrinsics=K, camera_group=g, n_groups=int(n_groups))


def focal_error(scene_scale, groups):
    """|sigma scale - 1| per group: how far the refined focal length is from the truth, relative"""
    return np.abs(np.asarray(groups, np.float64)[:, 0] * float(np.float32(scene_scale)) - 1.0)


def restate(s, refine=1, px=4.0, lambda0=1e-3, iterations=4, cg_iterations=8, cg_tol=0.1, dense=False, dense_first_step=False):
    """-> dict poses f32 [N, 12], points f32 [tcap, 4], intrinsics f32 [N, 4], groups f32 [n_groups, 3], obs_state [ocap] (-1
    where nothing is written), trace [iterations, 9], counts [5], near_tie (did a decision hang on less than the margins of
    tests/test_bundle_intr_twin.py), x0 / xg0 (the first step's camera and group updates), and with dense_first_step `dense` =
    (cameras, groups) of numpy.linalg.solve on the full damped normal equations of that step.  dense=True takes EVERY step from
    that solve instead of conjugate gradients (the reference of the recovery tests)."""
    act, usable, cam_free, T = cases.active_set(s)
    N = len(usable)
    NG = int(s.get("n_groups", 1))
    grp = np.zeros(N, np.int64) if s.get("camera_group") is None else np.asarray(s["camera_group"], np.uint32).astype(np.int64)
    thr2 = float(np.float32(px)) ** 2
    tol2 = float(np.float32(cg_tol)) ** 2
    lam = float(np.float32(lambda0))
    K0 = np.asarray(s["intrinsics"], np.float32).astype(np.float64)
    P0 = np.asarray(s["poses"], np.float32).astype(np.float64)
    R, tr = P0[:, :9].reshape(N, 3, 3).copy(), P0[:, 9:].copy()
    X = np.asarray(s["points"], np.float32).astype(np.float64)[:, :3].copy()
    op, ot, oi, orow = act.T if len(act) else (np.zeros(0, np.int64),) * 4
    xy = np.asarray(s["kps"], np.float32).astype(np.float64)[orow, :2]
    pt_free = np.zeros(len(X), bool)
    pt_free[ot] = True
    n = len(op)
    near = False
    in_group = grp < NG
    gsafe = np.where(in_group, grp, 0)
    grp_free = np.zeros(NG, bool)
    if refine:
        grp_free[np.unique(gsafe[oi][in_group[oi]])] = True
    fm, cm = bool(refine & 1), bool(refine & 2)
    pmask = np.array([fm, cm, cm])
    sig, dl = np.ones(NG), np.zeros((NG, 2))
    img_free_group = in_group & grp_free[gsafe]
    og = gsafe[oi]
    o_in_free = img_free_group[oi]

    def intrinsics(sig, dl):
        K = K0.copy()
        f = img_free_group
        K[f, 0], K[f, 1] = sig[gsafe[f]] * K0[f, 0], sig[gsafe[f]] * K0[f, 1]
        K[f, 2], K[f, 3] = K0[f, 2] + dl[gsafe[f], 0], K0[f, 3] + dl[gsafe[f], 1]
        return K

    def project(R, tr, X, K):
        q = np.einsum("nij,nj->ni", R[oi], X[ot])
        p = q + tr[oi]
        with np.errstate(all="ignore"):
            u = p[:, :2] / p[:, 2:3]
            e = K[oi, :2] * u + K[oi, 2:] - xy
        return q, p, u, e, (e * e).sum(1)

    def cost_of(R, tr, X, K):
        nonlocal near
        _, p, _, _, e2 = project(R, tr, X, K)
        inl = (p[:, 2] > 0) & (e2 <= thr2)
        near = near or bool((np.abs(e2 - thr2) <= 1e-9 * thr2).any())
        return float(np.where(inl, e2, thr2).sum()), inl

    trace = np.zeros((iterations, 9))
    x_first = xg_first = dense_out = None
    accepted = 0
    for it in range(iterations):
        K = intrinsics(sig, dl)
        q, p, u, e, e2 = project(R, tr, X, K)
        cost_k, inl = cost_of(R, tr, X, K)
        with np.errstate(all="ignore"):
            a, b = K[oi, 0] / p[:, 2], K[oi, 1] / p[:, 2]
        gx, gy = -a * u[:, 0], -b * u[:, 1]
        z, one = np.zeros(n), np.ones(n)
        Jx = np.stack([2 * gx * q[:, 1], 2 * (a * q[:, 2] - gx * q[:, 0]), -2 * a * q[:, 1], a, z, gx], 1)
        Jy = np.stack([2 * (gy * q[:, 1] - b * q[:, 2]), -2 * gy * q[:, 0], 2 * b * q[:, 0], z, b, gy], 1)
        Rr = R[oi]
        Px = a[:, None] * Rr[:, 0] + gx[:, None] * Rr[:, 2]
        Py = b[:, None] * Rr[:, 1] + gy[:, None] * Rr[:, 2]
        Gx = np.stack([K0[oi, 0] * u[:, 0] * fm, one * cm, z], 1)
        Gy = np.stack([K0[oi, 1] * u[:, 1] * fm, z, one * cm], 1)
        outer = lambda A, B, C, D: A[:, :, None] * B[:, None, :] + C[:, :, None] * D[:, None, :]
        Uo, Vo, Wo = outer(Jx, Jx, Jy, Jy), outer(Px, Px, Py, Py), outer(Jx, Px, Jy, Py)
        Go, Co, Wko = outer(Gx, Gx, Gy, Gy), outer(Jx, Gx, Jy, Gy), outer(Gx, Px, Gy, Py)
        gco, gpo, gko = Jx * e[:, :1] + Jy * e[:, 1:], Px * e[:, :1] + Py * e[:, 1:], Gx * e[:, :1] + Gy * e[:, 1:]
        keep = inl                                             # (outliers may hold NaNs: they add nothing)
        kg = inl & o_in_free
        U, gc = np.zeros((N, 6, 6)), np.zeros((N, 6))
        V, gp = np.zeros((len(X), 3, 3)), np.zeros((len(X), 3))
        G, gk = np.zeros((NG, 3, 3)), np.zeros((NG, 3))
        np.add.at(U, oi[keep], Uo[keep]), np.add.at(gc, oi[keep], gco[keep])
        np.add.at(V, ot[keep], Vo[keep]), np.add.at(gp, ot[keep], gpo[keep])
        np.add.at(G, og[kg], Go[kg]), np.add.at(gk, og[kg], gko[kg])
        n_in = np.bincount(ot[keep], minlength=len(X))
        g_in = np.bincount(og[kg], minlength=NG)
        for M in (U, V, G):
            d = np.einsum("nii->ni", M)
            d += lam * np.maximum(d, 1e-6)
        # the parameters not refined: the identity's rows, scaled by a refined parameter's damped diagonal entry
        s_d, c_d = G[:, 0, 0].copy(), G[:, 1, 1].copy()
        if not fm:
            G[:, 0, :], G[:, :, 0], gk[:, 0] = 0, 0, 0
            G[:, 0, 0] = c_d
        if not cm:
            G[:, 1:, :], G[:, :, 1:], gk[:, 1:] = 0, 0, 0
            G[:, 1, 1] = G[:, 2, 2] = s_d
        cam_moves = cam_free.copy()
        Uinv = np.zeros_like(U)
        for i in np.flatnonzero(cam_free):
            try:
                assert np.isfinite(U[i]).all()
                np.linalg.cholesky(U[i])
                Uinv[i] = np.linalg.inv(U[i])
            except (np.linalg.LinAlgError, AssertionError):
                cam_moves[i] = False
        with np.errstate(all="ignore"):
            det = np.linalg.det(V)
            mean = np.einsum("nii->n", V) / 3
            pt_moves = pt_free & (n_in >= 2) & (det > 1e-12 * mean ** 3)
            gdet = np.linalg.det(G) if NG else np.zeros(0)
            gmean = np.einsum("nii->n", G) / 3
            grp_moves = grp_free & (g_in > 0) & (gdet > 1e-12 * gmean ** 3)
            near = near or bool((grp_free & (g_in > 0) & (np.abs(gdet - 1e-12 * gmean ** 3) <= 1e-6 * np.abs(gdet))).any())
        Vinv = np.zeros_like(V)
        Vinv[pt_moves] = np.linalg.inv(V[pt_moves])
        Ginv = np.zeros_like(G)
        Ginv[grp_moves] = np.linalg.inv(G[grp_moves])
        cpl = inl & cam_moves[oi] & pt_moves[ot]
        kcpl = kg & grp_moves[og] & pt_moves[ot]
        ccpl = kg & grp_moves[og] & cam_moves[oi]

        def wt(vc, vk):                                        # per track: sum W^T v_c + W_k^T v_k
            out = np.zeros((len(X), 3))
            np.add.at(out, ot[cpl], np.einsum("nij,ni->nj", Wo[cpl], vc[oi[cpl]]))
            np.add.at(out, ot[kcpl], np.einsum("nij,ni->nj", Wko[kcpl], vk[og[kcpl]]))
            return out

        def w(y):                                              # per image: sum W y; per group: sum W_k y
            oc, ok_ = np.zeros((N, 6)), np.zeros((NG, 3))
            np.add.at(oc, oi[cpl], np.einsum("nij,nj->ni", Wo[cpl], y[ot[cpl]]))
            np.add.at(ok_, og[kcpl], np.einsum("nij,nj->ni", Wko[kcpl], y[ot[kcpl]]))
            return oc, ok_

        def cross(vc, vk):                                     # U_ck v_k per image, U_ck^T v_c per group
            oc, ok_ = np.zeros((N, 6)), np.zeros((NG, 3))
            np.add.at(oc, oi[ccpl], np.einsum("nij,nj->ni", Co[ccpl], vk[og[ccpl]]))
            np.add.at(ok_, og[ccpl], np.einsum("nij,ni->nj", Co[ccpl], vc[oi[ccpl]]))
            return oc, ok_

        solve_v = lambda b_: np.einsum("nij,nj->ni", Vinv, b_)
        solve_u = lambda b_: np.einsum("nij,nj->ni", Uinv, b_)
        solve_g = lambda b_: np.einsum("nij,nj->ni", Ginv, b_)
        mask, gmask = cam_moves[:, None], grp_moves[:, None] & pmask[None, :]

        def apply(pc, pk):
            yc, yk = w(solve_v(wt(pc, pk)))
            cc, ck = cross(pc, pk)
            return (np.where(mask, np.einsum("nij,nj->ni", U, pc) + cc - yc, 0.0),
                    np.where(gmask, np.einsum("nij,nj->ni", G, pk) + ck - yk, 0.0))

        yc, yk = w(solve_v(gp))
        rc, rk = np.where(mask, gc - yc, 0.0), np.where(gmask, gk - yk, 0.0)
        want_dense = dense or (it == 0 and dense_first_step)
        sol = _dense_step(U, V, G, Wo, Wko, Co, gc, gp, gk, cpl, kcpl, ccpl, oi, ot, og, cam_moves, pt_moves, grp_moves, pmask) \
            if want_dense else None
        x, xk = np.zeros((N, 6)), np.zeros((NG, 3))
        steps = 0
        if dense:
            x, xk = sol
        else:
            zc, zk = solve_u(rc), solve_g(rk)
            pc, pk = zc.copy(), zk.copy()
            rz = rz0 = float((rc * zc).sum()) + float((rk * zk).sum())
            for _ in range(cg_iterations):
                Ac, Ak = apply(pc, pk)
                pAp = float((pc * Ac).sum()) + float((pk * Ak).sum())
                if not (pAp > 0) or not (rz > 0):
                    break
                alpha = rz / pAp
                steps += 1
                x, xk, rc, rk = x + alpha * pc, xk + alpha * pk, rc - alpha * Ac, rk - alpha * Ak
                zc, zk = solve_u(rc), solve_g(rk)
                rz_new = float((rc * zc).sum()) + float((rk * zk).sum())
                beta, rz = rz_new / rz, rz_new
                if not (rz_new > 0) or rz_new <= tol2 * rz0:
                    break
                pc, pk = zc + beta * pc, zk + beta * pk
        if it == 0:
            x_first, xg_first = x.copy(), xk.copy()
            if dense_first_step:
                dense_out = sol
        dp = solve_v(gp - wt(x, xk))
        Rn, tn, Xn = R.copy(), tr.copy(), X.copy()
        for i in np.flatnonzero(cam_moves):
            Rn[i], tn[i] = cases.cayley(-x[i, :3]) @ R[i], tr[i] - x[i, 3:]
        Xn[pt_moves] = X[pt_moves] - dp[pt_moves]
        sn, dn = sig.copy(), dl.copy()
        gm = grp_moves
        if fm:
            sn[gm] = sig[gm] - xk[gm, 0]
        if cm:
            dn[gm] = dl[gm] - xk[gm, 1:]
        valid = bool((np.isfinite(sn[gm]) & (sn[gm] > 0)).all())
        near = near or bool((np.abs(sn[gm]) <= 1e-9).any())
        cost_new, _ = cost_of(Rn, tn, Xn, intrinsics(sn, dn))
        near = near or abs(cost_new - cost_k) <= 1e-12 * cost_k
        ok = valid and cost_new <= cost_k
        trace[it] = [cost_k, cost_new, lam, ok, steps, inl.sum(), (cam_free & ~cam_moves).sum(), (pt_free & ~pt_moves).sum(),
                     (grp_free & ~grp_moves).sum()]
        if ok:
            R, tr, X, sig, dl, accepted = Rn, tn, Xn, sn, dn, accepted + 1
            lam = max(lam / 4, 2.0 ** -40)
        else:
            lam = min(8 * lam, 2.0 ** 40)

    poses = np.asarray(s["poses"], np.float32).copy()
    poses[cam_free] = np.concatenate([R.reshape(N, 9), tr], 1).astype(np.float32)[cam_free]
    points = np.asarray(s["points"], np.float32).copy()
    points[pt_free, :3] = X.astype(np.float32)[pt_free]
    Kout = np.asarray(s["intrinsics"], np.float32).copy()
    Kout[img_free_group] = intrinsics(sig, dl).astype(np.float32)[img_free_group]
    state = np.full(len(s["obs_row"]), -1, np.int64)
    O = min(int(s["counts"][1]), len(s["obs_row"]))
    toff = np.minimum(np.asarray(s["track_offsets"], np.uint64), O).astype(np.int64)
    for t in range(T):
        state[toff[t]:max(toff[t], toff[t + 1])] = 0
    P32 = poses.astype(np.float64)
    _, p, _, _, e2 = project(P32[:, :9].reshape(N, 3, 3), P32[:, 9:], points[:, :3].astype(np.float64), Kout.astype(np.float64))
    near = near or bool((np.abs(e2 - thr2) <= 1e-9 * thr2).any())
    state[op] = np.where((p[:, 2] > 0) & (e2 <= thr2), 2, 1)
    inl = (p[:, 2] > 0) & (e2 <= thr2)
    return dict(poses=poses, points=points, intrinsics=Kout, groups=np.concatenate([sig[:, None], dl], 1).astype(np.float32),
                obs_state=state, trace=trace, near_tie=near, x0=x_first, xg0=xg_first, dense=dense_out,
                counts=np.array([cam_free.sum(), pt_free.sum(), n, accepted, grp_free.sum()]),
                rms=float(np.sqrt(e2[inl].mean())) if inl.any() else 0.0)


def _dense_step(U, V, G, Wo, Wko, Co, gc, gp, gk, cpl, kcpl, ccpl, oi, ot, og, cam_moves, pt_moves, grp_moves, pmask):
    """(cameras [N, 6], groups [NG, 3]) of numpy.linalg.solve on the dense damped normal equations over the moving cameras, the
    refined parameters of the moving groups and the moving points"""
    cams, grps, pts = np.flatnonzero(cam_moves), np.flatnonzero(grp_moves), np.flatnonzero(pt_moves)
    ci, gi, pi = ({c: k for k, c in enumerate(cams)}, {g: k for k, g in enumerate(grps)}, {p_: k for k, p_ in enumerate(pts)})
    nc, ng, npt = 6 * len(cams), 3 * len(grps), 3 * len(pts)
    H, g = np.zeros((nc + ng + npt,) * 2), np.zeros(nc + ng + npt)
    for c in cams:
        H[6 * ci[c]:6 * ci[c] + 6, 6 * ci[c]:6 * ci[c] + 6] = U[c]
        g[6 * ci[c]:6 * ci[c] + 6] = gc[c]
    for k_ in grps:
        a = nc + 3 * gi[k_]
        H[a:a + 3, a:a + 3] = G[k_]
        g[a:a + 3] = gk[k_]
    for p_ in pts:
        k = nc + ng + 3 * pi[p_]
        H[k:k + 3, k:k + 3] = V[p_]
        g[k:k + 3] = gp[p_]
    for k in np.flatnonzero(cpl):
        a, b = 6 * ci[oi[k]], nc + ng + 3 * pi[ot[k]]
        H[a:a + 6, b:b + 3] += Wo[k]
        H[b:b + 3, a:a + 6] += Wo[k].T
    for k in np.flatnonzero(kcpl):
        a, b = nc + 3 * gi[og[k]], nc + ng + 3 * pi[ot[k]]
        H[a:a + 3, b:b + 3] += Wko[k]
        H[b:b + 3, a:a + 3] += Wko[k].T
    for k in np.flatnonzero(ccpl):
        a, b = 6 * ci[oi[k]], nc + 3 * gi[og[k]]
        H[a:a + 6, b:b + 3] += Co[k]
        H[b:b + 3, a:a + 6] += Co[k].T
    sol = np.linalg.solve(H, g)
    xc, xk = np.zeros((len(cam_moves), 6)), np.zeros((len(grp_moves), 3))
    xc[cams] = sol[:nc].reshape(-1, 6)
    xk[grps] = sol[nc:nc + ng].reshape(-1, 3) * pmask
    return xc, xk
