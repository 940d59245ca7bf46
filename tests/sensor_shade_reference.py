"""TEST INFRASTRUCTURE -- float64 reference of the shaded-frame launch (include/lsim.h, lsim_sensor_shade), written from the header alone.

Built on the brute-force casts of tests/raycast_reference.py (every triangle of the mesh against every ray) and
tests/raycast_bodies_reference.py (forward kinematics, posed primitives, the analytic interval of each kind), imported unchanged.  It
shares no code with the kernel: the face of a hit is the brute force's own argmin, not a search around a stored range; the shadow ray is
one more brute-force cast, no grid walk and no bounding test.

Acceptance extends the nine-sample rule of raycast_reference: for the ray and its eight EPS_POS / EPS_ANG neighbours (the robot stays
where it is) the reference evaluates the face that is hit, its normal turned as the header says, and its light.
  * the normal under test must lie within tol_n (chord length, which is the angle for small ones) of the normal of ONE of the nine samples;
  * the light under test must equal the light of one of the nine; either light is accepted when |n . sun| <= tol_n for a sample;
  * a pixel is UNSTABLE when its nine samples disagree in label, in face or in light; at most raycast_reference.MAX_UNSTABLE of a scene's
    pixels may be, asserted on the reference alone before the value under test is looked at.  (A shadow edge is 2 * EPS_POS wide under
    this rule, against pixels of centimetres.)

The tolerances, fixed from the operation counts before the kernel was run (u = 2^-24, the fp32 unit roundoff):
  ANG_TOL = 2^-13 rad.  Terrain: a vertex coordinate (a + dx) * hs - border carries 2 u of its magnitude X, an edge vector the error of two
            vertices, 4 u X, relative to an edge of hs = 0.1 m: 40 u X per metre; the scenes here keep |X| <= 16 m (a 64 x 64 grid around the
            origin, heights of centimetres), so 640 u.  Each component of e1 x e2 is two products and a difference, 3 u of |e1| |e2| per
            edge error already counted twice (two edges): 1280 u + 3 u; the normalisation (a dot product, a reciprocal square root that the
            simulator's build does not round correctly, a product) changes the length by about 6 u and the direction by nothing.
            Bodies: the axes of a posed primitive are a rotation by the product of at most six fp32 quaternions (base, three joints with
            sinf / cosf of half an angle at 2 u each, the primitive's own): about 6 x 6 u = 36 u; the local normal into world orientation
            three products and two sums, 3 u.  The larger sum, 1283 u = 7.6e-5, rounded up to the next power of two: 2^-13 = 1.22e-4.
  curved primitives (sphere, capsule, the side of a cylinder): the normal turns with the hit point, by (position error of the hit) / radius.
            The position error of a sample is what raycast_bodies_reference allows its range, tol_k = ATOL + C_TOL * 2^-23 * (coordinate + t)
            / |n . d|, plus the sample step EPS_POS + EPS_ANG * t itself over |n . d| (a sideways step moves the hit along the surface by
            step / |n . d|): tol_n = ANG_TOL + (tol_k + 2 (EPS_POS + EPS_ANG t) / |n . d|) / radius.  Flat faces (box, caps, triangles): ANG_TOL.
  colour:   +-1 level per channel against the float64 formula applied to the launch's OWN surface, out and labels: the fp32 expression
            (a dozen roundings of values <= 1, under 2^-20) is off by far less than 1 / 255, so only a value at a rounding boundary moves.
            Terrain pixels whose P lies within EPS_POS + tol of a checker boundary are left out and count against MAX_UNSTABLE.

Mutants (MUTANTS): deliberately wrong variants of this reference; tests/test_sensor_shade.py asserts that each rejects the launch's output
on at least one scene -- the check can tell them apart.  The first one turns the terrain normal WITH the ray: merely leaving the turn out
cannot show, because over a height field without overhangs e1 x e2 of the header's two triangles points up or out of the riser, against
every ray that starts above the surface (the only origins the ray launch supports).
"""
import numpy as np

import raycast_bodies_reference as RB
import raycast_reference as REF

ANG_TOL = 2.0 ** -13
SHADOWS = 1
NUM_LABELS = 19
MUTANTS = ("normal_turned_with_the_ray", "sun_negated", "no_shadow_bias", "cap_for_side", "palette_off_by_one", "masked_bodies_cast_shadows")


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def terrain_faces(scene, o, d, near, far, chunk=1024):
    """brute force with the face kept: (t [M] (far: miss), raw unit normal e1 x e2 of the face [M, 3] (nan: miss), face index [M] (-1: miss))"""
    o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    M = o.shape[0]
    near, far = float(np.float32(near)), float(np.float32(far))
    t_out, n_out, f_out = np.full(M, far), np.full((M, 3), np.nan), np.full(M, -1, np.int64)
    if scene["mesh_type"] == 0 or scene["words"] is None:
        with np.errstate(divide="ignore", invalid="ignore"):
            t = -o[:, 2] / d[:, 2]
        ok = (np.abs(d[:, 2]) >= 1e-30) & (t >= near) & (t <= far)
        t_out[ok], n_out[ok], f_out[ok] = t[ok], [0.0, 0.0, 1.0], 0
        return t_out, n_out, f_out
    A, E1, E2 = REF.triangles(scene)
    Nn = np.cross(E1, E2)
    nn = (Nn * Nn).sum(1)
    G1, G2 = np.cross(E2, Nn) / nn[:, None], np.cross(Nn, E1) / nn[:, None]
    Nu = Nn / np.sqrt(nn)[:, None]
    na, ag1, ag2 = (Nu * A).sum(1), (A * G1).sum(1), (A * G2).sum(1)
    for c0 in range(0, M, chunk):
        oc, dc = o[c0:c0 + chunk], d[c0:c0 + chunk]
        nd = dc @ Nu.T
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (na[None, :] - oc @ Nu.T) / nd
            u = oc @ G1.T + t * (dc @ G1.T) - ag1[None, :]
            v = oc @ G2.T + t * (dc @ G2.T) - ag2[None, :]
            ok = (np.abs(nd) > 1e-14) & (u >= -1e-9) & (v >= -1e-9) & (u + v <= 1 + 1e-9) & (t >= near) & (t <= far)
        t = np.where(ok, t, np.inf)
        k = t.argmin(1)
        rows = np.arange(t.shape[0])
        hit = np.isfinite(t[rows, k])
        t_out[c0:c0 + chunk][hit] = t[rows, k][hit]
        n_out[c0:c0 + chunk][hit] = Nu[k][hit]
        f_out[c0:c0 + chunk][hit] = k[hit]
    return t_out, n_out, f_out


def prim_normal(kind, x, size, mutant=None):
    """(outward unit normal [.., 3] at the surface point x of a primitive in its own frame, face code [..], radius of curvature [..] (inf: flat))"""
    zero = 0.0 * x[..., 0]
    if kind == RB.SPHERE:
        return unit(x), zero.astype(np.int64), zero + size[0]
    if kind == RB.BOX:
        g = np.abs(x) - size[:3]
        k = g.argmax(-1)
        s = np.where(np.take_along_axis(x, k[..., None], -1)[..., 0] < 0, -1.0, 1.0)
        return s[..., None] * np.eye(3)[k], 2 * k + (s > 0), zero + np.inf
    if kind == RB.CYLINDER:
        rho = np.sqrt(x[..., 0] ** 2 + x[..., 1] ** 2)
        side = rho - size[0] >= np.abs(x[..., 2]) - size[1]
        if mutant == "cap_for_side":
            side = np.ones_like(side)
        sz = np.where(x[..., 2] < 0, -1.0, 1.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            ns = np.stack((x[..., 0] / rho, x[..., 1] / rho, zero), -1)
        n = np.where(side[..., None], ns, np.stack((zero, zero, sz), -1))
        return n, np.where(side, 0, 1 + (sz > 0)).astype(np.int64), np.where(side, size[0], np.inf)
    zc = np.clip(x[..., 2], -size[1], size[1])
    return unit(np.stack((x[..., 0], x[..., 1], x[..., 2] - zc), -1)), zero.astype(np.int64), zero + size[0]


def body_faces(prims, orel, d, near, far, mutant=None):
    """one env: (t [R] (far: none), label [R], world outward normal [R, 3], face id [R], radius [R]) over RB.posed_prims, the header's tie rule"""
    R = d.shape[0]
    t, label = np.full(R, far), np.zeros(R, np.int64)
    n, face, rad = np.full((R, 3), np.nan), np.full(R, -1, np.int64), np.full(R, np.inf)
    for i, (kind, body, c, axes, size) in enumerate(prims):
        ol, dl = (orel - c) @ axes.T, d @ axes.T
        ti, _ = RB.entry(kind, ol, dl, size)
        ok = (ti >= near) & (ti <= far) & ((ti < t) | (label == 0))
        if not ok.any():
            continue
        tt = np.where(ok, ti, 0.0)
        nl, fc, rr = prim_normal(kind, ol + tt[:, None] * dl, size, mutant)
        t, label = np.where(ok, ti, t), np.where(ok, 2 + body, label)
        n, face, rad = np.where(ok[:, None], nl @ axes, n), np.where(ok, 16 * i + fc, face), np.where(ok, rr, rad)
    return t, label, n, face, rad


def occluded(scene, prims, p, prel, sun, shadow_far):
    """one env: the shadow rays from p (world) / prel (base-relative) [R, 3] along sun over [0, shadow_far]"""
    _, _, lb, _ = RB.cast_bodies(prims, prel, np.broadcast_to(sun, prel.shape), 0.0, shadow_far)
    _, nd = REF.cast(scene, p, np.broadcast_to(sun, p.shape), 0.0, shadow_far)
    return (lb > 0) | ~np.isnan(nd)


def geometry(scene, robots, env_robot, root_states, dof_pos, o, orel, d, near, far, body_mask, mutant=None):
    """for given rays [N, R, 3], all that does not depend on the light: dict of label, t, n (turned), face, radius, win (a body), P, Prel"""
    near, far = float(np.float32(near)), float(np.float32(far))
    N, R = d.shape[:2]
    rs = np.asarray(root_states, np.float32).astype(np.float64)
    th = np.asarray(dof_pos, np.float32).astype(np.float64)
    tt, nt, ft = terrain_faces(scene, o.reshape(-1, 3), d.reshape(-1, 3), near, far)
    tt, nt, ft = tt.reshape(N, R), nt.reshape(N, R, 3), ft.reshape(N, R)
    away = (nt * d).sum(-1) > 0
    nt = np.where((~away if mutant == "normal_turned_with_the_ray" else away)[..., None], -nt, nt)
    g = {k: np.zeros((N, R)) for k in ("t", "radius")}
    g.update(label=np.zeros((N, R), np.int64), face=np.zeros((N, R), np.int64), win=np.zeros((N, R), bool), n=np.zeros((N, R, 3)), P=np.zeros((N, R, 3)),
             Prel=np.zeros((N, R, 3)), o=o, orel=orel, d=d)
    for e in range(N):
        prims = RB.posed_prims(robots[int(env_robot[e])], rs[e, 3:7], th[e], body_mask)
        tb, lb, nb, fb, rb = body_faces(prims, orel[e], d[e], near, far, mutant)
        win = (lb > 0) & (tb <= tt[e])
        label = np.where(win, lb, np.where(ft[e] >= 0, 1, 0))
        t = np.where(win, tb, tt[e])
        n = np.where((label > 0)[:, None], np.where(win[:, None], nb, nt[e]), 0.0)
        g["label"][e], g["t"][e], g["n"][e], g["face"][e], g["win"][e], g["radius"][e] = label, t, n, np.where(win, fb, ft[e]), win, np.where(win, rb, np.inf)
        g["P"][e], g["Prel"][e] = o[e] + t[:, None] * d[e], orel[e] + t[:, None] * d[e]
    return g


def lighting(g, scene, robots, env_robot, root_states, dof_pos, body_mask, shade, mutant=None):
    """the geometry `g` with light, c = n . sun and tol_n [N, R] added (a new dict)"""
    rs = np.asarray(root_states, np.float32).astype(np.float64)
    th = np.asarray(dof_pos, np.float32).astype(np.float64)
    sun = np.asarray(shade["sun"], np.float32).astype(np.float64)
    if mutant == "sun_negated":
        sun = -sun
    bias, sfar = (float(np.float32(shade[k])) for k in ("shadow_bias", "shadow_far"))
    if mutant == "no_shadow_bias":
        bias = 0.0
    n, t, hit = g["n"], g["t"], g["label"] > 0
    c = (n * sun).sum(-1)
    light = (hit & (c > 0)).astype(np.float64)
    if shade["flags"] & SHADOWS:
        for e in range(c.shape[0]):
            lit = light[e] > 0
            if lit.any():
                casters = RB.posed_prims(robots[int(env_robot[e])], rs[e, 3:7], th[e], 0x1FFFF if mutant == "masked_bodies_cast_shadows" else body_mask)
                occ = occluded(scene, casters, (g["P"][e] + bias * n[e])[lit], (g["Prel"][e] + bias * n[e])[lit], sun, sfar)
                light[e][np.flatnonzero(lit)[occ]] = 0.0
    nd = np.maximum(np.abs((n * g["d"]).sum(-1)), 1e-300)
    coord = np.where(g["win"], np.maximum(np.abs(g["orel"]).max(-1), np.abs(g["Prel"]).max(-1)), np.maximum(np.abs(g["o"]).max(-1), np.abs(g["P"]).max(-1)))
    pos = REF.ATOL + REF.C_TOL * 2.0 ** -23 * (coord + t) / nd + 2.0 * (REF.EPS_POS + REF.EPS_ANG * t) / nd
    return dict(g, light=light, c=c, tol_n=ANG_TOL + np.where(hit, pos / g["radius"], 0.0))


def geometries(scene, robots, env_robot, root_states, dof_pos, mount, dirs, near, far, body_mask=0x1FFFF, flags=0, mutant=None):
    """geometry() of the nine samples: what a scene's suns and flags share"""
    return [geometry(scene, robots, env_robot, root_states, dof_pos, o, orel, d, near, far, body_mask, mutant) for o, orel, d in samples(root_states, mount, dirs, flags)]


def samples(root_states, mount, dirs, flags):
    """the nine (o, o', d) of raycast_bodies_reference.envelope, the centre first"""
    o, orel, d = RB.rays(root_states, mount, dirs, flags)
    N, R = d.shape[:2]
    b1, b2 = (b.reshape(N, R, 3) for b in REF._transverse(d.reshape(-1, 3)))
    out = [(o, orel, d)]
    for b in (b1, b2):
        for sgn in (1.0, -1.0):
            out.append((o + sgn * REF.EPS_POS * b, orel + sgn * REF.EPS_POS * b, d))
            dd = d + sgn * REF.EPS_ANG * b
            out.append((o, orel, dd / np.linalg.norm(dd, axis=-1, keepdims=True)))
    return out


def nine(scene, robots, env_robot, root_states, dof_pos, mount, dirs, near, far, shade, body_mask=0x1FFFF, flags=0, mutant=None, geoms=None):
    """the nine evaluations and which pixels are stable (label, face and light agree); `geoms`: geometries() of the same arguments, kept by the caller"""
    if geoms is None:
        geoms = geometries(scene, robots, env_robot, root_states, dof_pos, mount, dirs, near, far, body_mask, flags, mutant)
    ev = [lighting(g, scene, robots, env_robot, root_states, dof_pos, body_mask, shade, mutant) for g in geoms]
    stable = np.ones(ev[0]["label"].shape, bool)
    for s in ev[1:]:
        stable &= (s["label"] == ev[0]["label"]) & (s["face"] == ev[0]["face"]) & (s["light"] == ev[0]["light"])
    return ev, stable


def palette_rgb(palette):
    p = np.asarray(palette).astype(np.uint32)
    return np.stack((p & 255, (p >> 8) & 255, (p >> 16) & 255), -1).astype(np.float64) / 255.0


def colours(P, n, light, labels, shade, palette, mutant=None):
    """the header's colour formula in float64: uint8 [.., 3] and, per pixel, the distance of P to the nearest checker boundary (inf: none)"""
    sun = np.asarray(shade["sun"], np.float32).astype(np.float64)
    amb, chk, gain = (float(np.float32(shade[k])) for k in ("ambient", "checker", "checker_gain"))
    labels = np.asarray(labels).astype(np.int64)
    labels = np.where(labels >= NUM_LABELS, 0, labels)
    idx = np.minimum(labels + 1, NUM_LABELS - 1) if mutant == "palette_off_by_one" else labels
    a = palette_rgb(palette)[idx]
    k = amb + (1.0 - amb) * light * (n * sun).sum(-1)
    edge = np.full(labels.shape, np.inf)
    if chk > 0.0:
        cell = P[..., :2] / chk
        odd = (np.floor(cell[..., 0]) + np.floor(cell[..., 1])) % 2 == 1
        a = np.where(((labels == 1) & odd)[..., None], a * gain, a)
        edge = np.where(labels == 1, (np.abs(cell - np.round(cell)) * chk).min(-1), np.inf)
    k = np.where(labels == 0, 1.0, k)
    return np.floor(255.0 * np.clip(a * k[..., None], 0.0, 1.0) + 0.5).astype(np.int64), edge


def check(scene, robots, env_robot, root_states, dof_pos, mount, dirs, near, far, shade, palette, rgba, surface, out, labels, scale=None,
          body_mask=0x1FFFF, flags=0, label="", mutant=None, strict=True, ref=None):
    """assert the cap on unstable pixels on the reference alone; then the launch's surface [N, R, 4] against the nine samples and its rgba
    [N, R] words against the colour formula on its own surface, out [N, R] and labels [N, R].  strict: every pixel must pass; otherwise the
    shares of failing pixels must stay within MAX_UNSTABLE.  `ref`: nine() of the same arguments, kept by the caller.  Returns dict(unstable, normal, light, dark_terrain: shares / counts)"""
    ev, stable = ref if ref is not None else nine(scene, robots, env_robot, root_states, dof_pos, mount, dirs, near, far, shade, body_mask, flags, mutant)
    N, R = stable.shape
    c0 = ev[0]
    sc = np.ones(R) if scale is None else np.asarray(scale, np.float32).astype(np.float64)
    o, _, d = RB.rays(root_states, mount, dirs, flags)
    gl = np.asarray(labels).astype(np.int64)
    g_out = np.asarray(out, np.float64)
    Pg = o + (g_out / sc[None, :])[..., None] * d
    surf = np.asarray(surface, np.float64)
    # how far the launch's P may lie from the point its colour is checked at: the sample step plus the range's tolerance, along the surface
    pos_tol = (REF.EPS_POS + REF.ATOL + REF.C_TOL * 2.0 ** -23 * (np.abs(Pg).max(-1) + g_out)) / np.maximum(np.abs((surf[..., :3] * d).sum(-1)), 1e-3)
    want_rgb, edge = colours(Pg, surf[..., :3], surf[..., 3], gl, shade, palette, mutant)
    near_edge = edge <= pos_tol
    share = 1.0 - (stable & ~near_edge).mean()
    dark = int(((c0["label"] == 1) & (c0["c"] > 0) & (c0["light"] == 0) & stable).sum())
    print(f"sensor shade {label}: {N * R} pixels, unstable share {share:.4%} (checker edge {near_edge.mean():.4%}), terrain {np.mean(c0['label'] == 1):.2%}, "
          f"body {np.mean(c0['label'] >= 2):.2%}, lit {np.mean(c0['light'] > 0):.2%}, dark terrain facing the sun {dark}")
    assert share <= REF.MAX_UNSTABLE, (label, share)
    assert np.isfinite(surf).all(), label
    ok_n, ok_l = np.zeros((N, R), bool), np.zeros((N, R), bool)
    for s in ev:
        same = s["label"] == gl
        ok_n |= same & (np.linalg.norm(surf[..., :3] - s["n"], axis=-1) <= s["tol_n"])
        ok_l |= same & ((surf[..., 3] == s["light"]) | ((np.abs(s["c"]) <= s["tol_n"]) & (s["label"] > 0)))
    bad_n, bad_l = ~ok_n, ~ok_l
    got = np.asarray(rgba).astype(np.uint32)
    got_rgb = np.stack((got & 255, (got >> 8) & 255, (got >> 16) & 255), -1).astype(np.int64)
    bad_c = (np.abs(got_rgb - want_rgb).max(-1) > 1) & ~near_edge
    bad_a = (got >> 24) != 255
    res = {"unstable": share, "normal": bad_n.mean(), "light": bad_l.mean(), "colour": bad_c.mean(), "dark_terrain": dark}
    print(f"sensor shade {label}: normals beyond tolerance {res['normal']:.4%}, lights that differ {res['light']:.4%}, colours off by more than 1 {res['colour']:.4%}")
    for what, bad in (("normal", bad_n), ("light", bad_l), ("colour", bad_c), ("alpha", bad_a)):
        limit = 0.0 if strict or what in ("colour", "alpha") else REF.MAX_UNSTABLE
        if bad.mean() > limit:
            k = np.argwhere(bad)[:5]
            raise AssertionError(f"{label}: {what} wrong on {bad.sum()} of {bad.size} pixels; first: " + "; ".join(
                f"env {e} pixel {r}: label {gl[e, r]} (ref {c0['label'][e, r]}), surface {surf[e, r]}, ref n {c0['n'][e, r]} light {c0['light'][e, r]} "
                f"c {c0['c'][e, r]:.3g}, rgb {got_rgb[e, r]} want {want_rgb[e, r]}" for e, r in k))
    return res
