"""An independent second opinion on one shading round (test infrastructure).

Written from the reference's GLSL alone -- raytracing/rayshading.comp:25-28,48-278 (composite, the chain walk :60-116 and the rest
of main), raytracing/surface.comp:81-161,165-195 (validateTexture, the fetch* functions, getNormalMapping, main),
raytracing/directTraverse.comp:116-217 (interpolateMeshData, texcoords and tangent included), public/environment.glsl:23-26,58-60
(readEnv), include/shadinglib.glsl, include/rayslib.glsl:59-203, include/random.glsl -- in plain Python with numpy float32 scalars
and numpy's own sin / cos / pow / sqrt / arctan2 / arcsin, NOT from oracle/psm_oracle_shade.c and not through the pinned polynomials
of psm_math.h. It covers a frame of any scene the product renders: hit chains of any length with hits outside the material window
(not actived: surface.comp:172-173,190-194), textures in every part, both branches of getNormalMapping, any number of lights, a
constant sky colour or an equirect sky image.

Canonical rules it shares with the oracle by construction: the "RNG stream id" row (the ray's path key; child keys),
the "next-queue order" row ([current, diffuse, reflection, shadow] per input ray), the "radiance accumulation" row (a per-texel sum),
the "M.v, dot, normalize, cross" row, and the "materials / sky" row as written, in float32 -- the one thing GL leaves to the
implementation: texel = c / 255, the stated bilinear association, GL_REPEAT for material textures, clamp to edge for the sky, a
non-finite coordinate reads 0. With that rule a fetched value cannot round differently between the two readings, so neither can
its fp16 packing. Not modelled: a hit record's stale `bitfield` (interpolateMeshData leaves HitActived as the slot's last user set
it; here a hit is actived exactly when surface.comp's main writes it).

shade_round(..., texcoords=None, textures=None, skybox=None, material_offset=None, stats=None)
    -> (list of output ray tuples (origin, direct, color, bitfield, texel, path key, index of the input ray), {texel: [r, g, b, deposits]})
"""
import numpy as np

F = np.float32
PZERO = F(0.0005)
INF = F(10000.0)
GAP = F(PZERO * F(2.0))
TWO_PI = F(6.2831853071795864769252867665590057683943)
SQRT13 = F(0.5773502691896257645091487805019574556476)
U32 = 0xFFFFFFFF


def hash32(x):
    x = (x + (x << 10)) & U32
    x ^= x >> 6
    x = (x + (x << 3)) & U32
    x ^= x >> 11
    x = (x + (x << 15)) & U32
    return x


class Rng:  # random(), include/random.glsl:37-46, with globalInvocationSMP = the path key
    def __init__(self, smp, time):
        self.smp, self.clocks, self.t5 = smp & U32, 0, (time << 5) & U32

    def next(self):
        hs = self.clocks
        self.clocks = hash32((self.clocks + 1) & U32)
        h = hash32(self.smp ^ hash32(hs) ^ hash32(self.t5))
        f = np.array([(h & 0x007FFFFF) | 0x3F800000], np.uint32).view(np.float32)[0]
        return F(f - np.floor(f))  # fract


def v3(x, y, z):
    return np.array([x, y, z], np.float32)


def dot(a, b):
    return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))


def normalize(a):
    return (a * F(F(1.0) / F(np.sqrt(dot(a, a))))).astype(np.float32)


def cross(a, b):
    return v3(F(a[1] * b[2]) - F(b[1] * a[2]), F(a[2] * b[0]) - F(b[2] * a[0]), F(a[0] * b[1]) - F(b[0] * a[1]))


def mix(x, y, a):
    return (x * (F(1.0) - a) + y * a).astype(np.float32) if isinstance(x, np.ndarray) else F(F(x * F(F(1.0) - a)) + F(y * a))


def clamp(x, lo, hi):
    return np.minimum(np.maximum(x, F(lo)), F(hi)).astype(np.float32) if isinstance(x, np.ndarray) else min(max(x, F(lo)), F(hi))


def mlength(c):
    return max(c[0], max(c[1], c[2]))


def half(x):  # packHalf + unpackHalf round trip
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def bf(b, off, bits):
    return (b >> off) & ((1 << bits) - 1)


def bfs(b, v, off, bits):
    m = ((1 << bits) - 1) << off
    return (b & ~m) | ((v << off) & m)


ACT, TYPE, DL, TARGET, BOUNCE, BASIS = (0, 1), (1, 2), (3, 1), (4, 4), (8, 4), (12, 1)


class Ray:
    def __init__(self, origin, direct, color, final, b, texel):
        self.origin, self.direct, self.color, self.final, self.b, self.texel = origin, direct, color, final, int(b), int(texel)

    def copy(self):
        return Ray(self.origin.copy(), self.direct.copy(), self.color.copy(), self.final.copy(), self.b, self.texel)

    def get(self, f):
        return bf(self.b, *f)

    def set(self, f, v):
        self.b = bfs(self.b, int(v), *f)


def random_cosine(g, normal):  # random.glsl:48-69
    up = F(np.sqrt(g.next()))
    over = F(np.sqrt(F(F(1.0) - F(up * up))))
    around = F(g.next() * TWO_PI)
    p0 = v3(0, 0, 1)
    if abs(normal[0]) < SQRT13:
        p0 = v3(1, 0, 0)
    elif abs(normal[1]) < SQRT13:
        p0 = v3(0, 1, 0)
    p1 = normalize(cross(normal, p0))
    p2 = cross(normal, p1)
    ca, sa = F(F(np.cos(around)) * over), F(F(np.sin(around)) * over)
    return normalize((normal * up + (p1 * ca + p2 * sa)).astype(np.float32))


def random_direction_in_sphere(g):  # random.glsl:71-76
    up = F(F(g.next() * F(2.0)) - F(1.0))
    over = F(np.sqrt(F(F(1.0) - F(up * up))))
    around = F(g.next() * TWO_PI)
    return normalize(v3(up, F(F(np.cos(around)) * over), F(F(np.sin(around)) * over)))


def light_center(L):  # shadinglib.glsl:22-26
    lv = np.asarray(L["lightVector"], np.float32)
    lvec = normalize(lv[:3]) * (F(-1.0) if lv[1] < 0 else F(1.0))
    return (lvec * lv[3] + np.asarray(L["lightOffset"], np.float32)[:3]).astype(np.float32)


def intersect_sphere(origin, ray, centre, radius):  # shadinglib.glsl:32-48
    ts = (origin - centre).astype(np.float32)
    a = dot(ray, ray)
    b = F(F(2.0) * dot(ts, ray))
    c = F(dot(ts, ts) - F(radius * radius))
    disc = F(F(b * b) - F(F(F(4.0) * a) * c))
    t = INF
    if disc > 0:
        da = F(F(0.5) / a)
        sq = F(np.sqrt(disc))
        t1, t2 = F(F(-b - sq) * da), F(F(-b + sq) * da)
        mn, mx = min(t1, t2), max(t1, t2)
        if mx >= 0:
            t = mn if mn >= 0 else mx
    return t


class Sink:
    """queue + per-texel sums: createRay / storeRay / _collect (rayslib.glsl:59-203)"""

    def __init__(self):
        self.out, self.tex, self.it = [], {}, -1

    def collect(self, ray):
        c = np.maximum(ray.final, F(0.0))
        if mlength(c) < F(10000.0) and not np.isnan(c).any() and not np.isinf(c).any():
            s = self.tex.setdefault(ray.texel, [0.0, 0.0, 0.0, 0])
            s[0] += float(c[0]); s[1] += float(c[1]); s[2] += float(c[2]); s[3] += 1
        ray.final = v3(0, 0, 0)

    def create_ray(self, ray, pkey):  # createRay -> createRayStrict (`in` parameter: works on a copy)
        ray = ray.copy()
        invalid = ray.get(ACT) == 0 or ray.get(BOUNCE) <= 0 or mlength(ray.color) < F(0.0001)
        if mlength(ray.final) >= F(0.0001) and ray.get(ACT) == 0:
            self.collect(ray)
        ray.set(BASIS, 0)
        if invalid:
            return
        ray.set(BOUNCE, ray.get(BOUNCE) - 1)
        self.out.append((ray.origin.copy(), ray.direct.copy(), ray.color.copy(), ray.b, ray.texel, pkey, self.it))


def child_key(pkey, site):
    return hash32(pkey ^ hash32(site))


def fetch_texel(img, u, v, ox=0, oy=0, repeat=True):
    """texture() of an RGBA8 image [h, w, 4] (row 0 = v 0) by the rule of DESIGN.md 2.1, "materials / sky", as written, in float32:
    texel = c / 255, weights a, b from coordinate * size - 0.5 (material textures: of fract(coordinate), GL_REPEAT; the sky: clamp
    to edge), (t00 (1 - a) + t10 a) (1 - b) + (t01 (1 - a) + t11 a) b; a non-finite coordinate reads 0 (surface.comp:85-95)"""
    h, w = img.shape[0], img.shape[1]
    with np.errstate(all="ignore"):
        u, v = F(F(u) + F(F(ox) / F(w))), F(F(v) + F(F(oy) / F(h)))              # :92
        if not (np.isfinite(u) and np.isfinite(v)):
            return np.zeros(4, np.float32)
        if repeat:
            u, v = F(u - np.floor(u)), F(v - np.floor(v))
        x, y = F(F(u * F(w)) - F(0.5)), F(F(v * F(h)) - F(0.5))
    fx, fy = np.floor(x), np.floor(y)
    a, b = F(x - fx), F(y - fy)
    x0, y0 = int(fx), int(fy)
    x1, y1 = x0 + 1, y0 + 1
    if repeat:
        x0, x1, y0, y1 = x0 % w, x1 % w, y0 % h, y1 % h
    else:
        x0, x1, y0, y1 = min(max(x0, 0), w - 1), min(max(x1, 0), w - 1), min(max(y0, 0), h - 1), min(max(y1, 0), h - 1)
    t00, t10, t01, t11 = [(img[yy, xx].astype(np.float32) / F(255.0)).astype(np.float32) for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1))]
    top = (t00 * F(F(1.0) - a) + t10 * a).astype(np.float32)
    bot = (t01 * F(F(1.0) - a) + t11 * a).astype(np.float32)
    return (top * F(F(1.0) - b) + bot * b).astype(np.float32)


def valid_texture(textures, binding):  # validateTexture, surface.comp:81-83
    binding = int(binding) & U32
    return binding != 0 and binding != U32 and binding < 32 and textures is not None and textures.get(binding) is not None \
        and textures[binding].shape[1] > 0


def equal_f(a, b):  # mathlib.glsl:14
    return abs(F(a - b)) < PZERO


def close_call(a, b):
    """a tolerant compare of a and b that is decided within 1e-5 of its threshold"""
    return abs(abs(float(F(a - b))) - float(PZERO)) < 1e-5


def read_env(skybox, sky, r, note):  # environment.glsl:23-26,58-60
    if skybox is None:
        return np.asarray(sky, np.float32)[:3]
    note("sky_lookup", count_only=True)
    pi = F(3.1415926535897932384626422832795028841971)
    nr = normalize(r)
    with np.errstate(all="ignore"):
        u = F(np.float64(F(F(np.arctan2(nr[2], nr[0])) / pi)) * 0.5 + 0.5)       # fma(vec2(atan, asin * 2) / PI, 0.5, 0.5)
        v = F(np.float64(F(F(F(np.arcsin(nr[1])) * F(2.0)) / pi)) * 0.5 + 0.5)
    if min(float(u), 1.0 - float(u)) < 1e-4:
        note("sky_seam")
    return fetch_texel(skybox, u, v, repeat=False)[:3]


def interpolate(h, tris, normals, texcoords):
    """interpolateMeshData, directTraverse.comp:116-217 -> (normal, tangent, texcoord, t)"""
    u, v, t, tri = F(h["u"]), F(h["v"]), F(h["t"]), int(h["tri"])
    p = tris[tri]
    vs = v3(F(F(F(1.0) - u) - v), u, v)
    d1, d2 = (p[1] - p[0]).astype(np.float32), (p[2] - p[0]).astype(np.float32)
    nor = normalize(cross(d1, d2))
    tn = normals[tri]
    nrm = v3(*[F(F(F(vs[0] * tn[0][k]) + F(vs[1] * tn[1][k])) + F(vs[2] * tn[2][k])) for k in range(3)])
    nrm = normalize(nrm)  # lessF(length, 0) never holds
    nrm = (nrm * np.sign(dot(nrm, nor))).astype(np.float32)
    tc = np.zeros((3, 2), np.float32) if texcoords is None else np.asarray(texcoords[tri], np.float32)
    texcoord = [F(F(F(vs[0] * tc[0][c]) + F(vs[1] * tc[1][c])) + F(vs[2] * tc[2][c])) for c in range(2)]     # :209
    dl0 = [F(tc[1][0] - tc[0][0]), F(tc[2][0] - tc[0][0])]                      # :191-197
    dv = [F(tc[1][1] - tc[0][1]), F(tc[2][1] - tc[0][1])]
    dl1 = [F(dv[1] * F(1.0)), F(dv[0] * F(-1.0))]
    if abs(dl0[0]) < F(0.000001) and abs(dl0[1]) < F(0.000001):
        dl0 = [F(1.0), F(0.0)]
    if abs(dl1[0]) < F(0.000001) and abs(dl1[1]) < F(0.000001):
        dl1 = [F(1.0), F(0.0)]
    f = F(F(1.0) / F(F(dl0[0] * dl1[0]) + F(dl0[1] * dl1[1])))                  # :199-201
    if np.isnan(f):
        f = F(0.0)
    if np.isinf(f):
        f = F(10000.0)
    tang = v3(*[F(F(np.float64(dl1[0]) * np.float64(d1[k]) + np.float64(F(dl1[1] * d2[k]))) * f) for k in range(3)])   # :203, fma
    tangent = normalize((tang - nrm * np.sign(dot(tang, nor))).astype(np.float32))
    return nrm, tangent, texcoord, t


def surface(m, nrm, tangent, texcoord, textures, note):
    """surface.comp:102-161,176-189 for an actived hit -> (albedo, emission, metallicRoughness, normal), the three as packHalf leaves them"""
    tu, tv = texcoord

    def fetch(part, default, ox=0, oy=0):
        return fetch_texel(textures[int(m[part]) & U32], tu, tv, ox, oy) if valid_texture(textures, m[part]) else default
    nh = normalize(nrm)
    tg = normalize(tangent)
    bt = normalize(cross(nh, tg))
    flat = np.array([0.5, 0.5, 1.0, 1.0], np.float32)
    tc = fetch("bumpPart", flat)                                                # getNormalMapping, :138-153
    if valid_texture(textures, m["bumpPart"]) and (close_call(tc[0], tc[1]) or (equal_f(tc[0], tc[1]) and close_call(tc[0], tc[2]))):
        note("normal_map_kind")
    if equal_f(tc[0], tc[1]) and equal_f(tc[0], tc[2]):
        note("height_map", count_only=True)
        p00 = v3(0, 0, F(fetch("bumpPart", flat, 0, 0)[0] * F(2.0)))
        p01 = v3(1, 0, F(fetch("bumpPart", flat, 1, 0)[0] * F(2.0)))
        p10 = v3(0, 1, F(fetch("bumpPart", flat, 0, 1)[0] * F(2.0)))
        nm = normalize(cross((p01 - p00).astype(np.float32), (p10 - p00).astype(np.float32)))
    else:
        if valid_texture(textures, m["bumpPart"]):
            note("normal_map", count_only=True)
        y = (tc[:3] * F(2.0) + F(-1.0)).astype(np.float32)                      # fma(tc, 2, -1): the product is exact
        nm = normalize((v3(0, 0, 1) * F(0.0) + y * F(1.0)).astype(np.float32))  # mix(., ., 1)
    nm = normalize(nm)                                                          # :186
    shn = normalize((tg * nm[0] + bt * nm[1] + nh * nm[2]).astype(np.float32))
    diffuse = fetch("diffusePart", np.maximum(np.array([m["diffuse"][0], m["diffuse"][1], m["diffuse"][2], 1.0], np.float32), F(0.0)))
    emi = fetch("emissivePart", np.zeros(4, np.float32))
    spc = fetch("specularPart", np.asarray(m["specular"], np.float32))
    albedo = half(diffuse)
    emission = half(np.array([emi[0] * F(2.0), emi[1] * F(2.0), emi[2] * F(2.0), 1.0], np.float32))
    mr = half(np.array([spc[1], spc[2], 0.0, 0.0], np.float32))
    return albedo, emission, mr, shn


def composite(src, dst):  # rayshading.comp:25-28
    with np.errstate(all="ignore"):
        oa = F(src[3] + F(dst[3] * F(F(1.0) - src[3])))
        rgb = ((src[:3] * src[3] + (dst[:3] * dst[3]).astype(np.float32) * F(F(1.0) - src[3])).astype(np.float32) / max(oa, F(0.00001))).astype(np.float32)
    return clamp(np.array([rgb[0], rgb[1], rgb[2], oa], np.float32), 0.0, 1.0)


BRANCHES = ("first_inactive_later_active", "none_active", "composite_partial", "early_stop", "inactive_skipped", "layer_break",
            "height_map", "normal_map", "sky_lookup")


def shade_round(tris, normals, tri_mats, materials, mat_offset, lights, sky, time, rays, hits, counts, texcoords=None, textures=None,
                skybox=None, material_offset=None, stats=None):
    """stats, if given, is a dict the round fills: per name in BRANCHES the number of rays that took that branch of
    rayshading.comp:60-116 / surface.comp:138-153 at least once (and "sky_lookup": read the sky image), "close_rays" the input rays for which a discrete decision fell
    within 1e-5 of its threshold (an equalF, the albedo.a > 0.99999 stop) or whose sky lookup lies within 1e-4 of the u = 0 / 1
    seam, "close_texels" the texels those rays deposit into. Each output ray tuple ends with the index of its input ray."""
    if material_offset is not None:
        mat_offset = material_offset
    sink = Sink()
    nmat = len(materials)
    if stats is not None:
        for k in BRANCHES:
            stats.setdefault(k, 0)
        stats.setdefault("close_rays", set())
        stats.setdefault("close_texels", set())
    taken = set()

    def flush():
        if stats is not None:
            for k in taken:
                if k in stats:
                    stats[k] += 1
    for it in range(rays.shape[0]):
        flush()
        r = rays[it]
        ray = Ray(np.array(r["origin"], np.float32), np.array(r["direct"], np.float32), np.array(r["color"], np.float32),
                  v3(0, 0, 0), r["bitfield"], r["texel"])
        pkey = int(r["pkey"])
        g = Rng(pkey, time)
        n = int(counts[it])
        skipping = False
        sink.it = it
        taken = set()

        def note(what, count_only=False):
            taken.add(what)
            if not count_only and stats is not None:
                stats["close_rays"].add(it)
                stats["close_texels"].add(int(r["texel"]))
        # ---- the chain: interpolateMeshData (directTraverse.comp:116-217) and surface.comp:165-195 per hit, then rayshading.comp:60-116
        albedo = emission = mr = np.zeros(4, np.float32)
        normal_h = v3(0, 0, 0)
        uvt_t = INF
        if n > 0:
            chain = []
            for k in range(n):
                nrm, tangent, texcoord, t = interpolate(hits[it, k], tris, normals, texcoords)
                mat_id = int(tri_mats[int(hits[it, k]["tri"])]) - mat_offset
                chain.append((0 <= mat_id < nmat, mat_id, nrm, tangent, texcoord, t))    # actived: surface.comp:172-173,190-194
            at = 0
            while not chain[at][0] and at + 1 < n:                                     # :69-71
                at += 1
            if at > 0 and chain[at][0]:
                taken.add("first_inactive_later_active")
            active, mat_id, nrm, tangent, texcoord, uvt_t = chain[at]
            nxt = at + 1
            if not active:                                                             # :73-79: transparent, keeps the traversal normal
                taken.add("none_active")
                normal_h = nrm
                nxt = n
            else:
                albedo, emission, mr, normal_h = surface(materials[mat_id], nrm, tangent, texcoord, textures, note)
            while nxt < n:                                                             # :92-116
                active, mat_id, nrm, tangent, texcoord, t = chain[nxt]
                if close_call(uvt_t, t):
                    note("layer_distance")
                if not equal_f(uvt_t, t):
                    taken.add("layer_break")
                    break
                if not active:
                    taken.add("inactive_skipped")
                    nxt += 1
                    continue
                h_albedo, h_emission, h_mr, h_normal = surface(materials[mat_id], nrm, tangent, texcoord, textures, note)
                if F(0.0) < albedo[3] < F(1.0):
                    taken.add("composite_partial")
                uvt_t = t
                albedo = composite(albedo, h_albedo)
                normal_h = mix(normal_h, h_normal, h_albedo[3])
                mr = mix(mr, h_mr, h_albedo[3])
                emission = mix(emission, h_emission, h_albedo[3])
                if abs(float(F(albedo[3] - F(0.99999)))) < 1e-5:          # (an alpha of exactly 1 is 1.0014e-5 above the float 0.99999)
                    note("filled")
                if albedo[3] > F(0.99999):
                    taken.add("early_stop")
                    break
                nxt += 1
        # ---- physical lights (:119-138)
        lc = -1
        typ = ray.get(TYPE)
        if ray.get(DL) > 0 and typ in (1, 2) and not skipping:
            for i in range(min(len(lights), 16)):
                dt = intersect_sphere(ray.origin, ray.direct, light_center(lights[i]), F(F(lights[i]["lightColor"][3]) + GAP))
                t = F(F(1.0) * dt)
                if F(INF - dt) >= PZERO and F(uvt_t - t) > -PZERO:
                    lc = i
        if lc >= 0 and (ray.get(TARGET) == lc or typ != 2):
            ray.final = (ray.color * np.maximum(np.asarray(lights[lc]["lightColor"], np.float32)[:3], F(0.0))).astype(np.float32)
            ray.color = (ray.color * F(0.0)).astype(np.float32)
            ray.set(ACT, 0)
            skipping = True
        # ---- background (:141-152); EnvironmentShader reads the direction before :155 normalises it (readEnv normalises its own)
        env = read_env(skybox, sky, ray.direct, note) if (F(uvt_t - INF) > -PZERO and typ != 2 and not skipping) else None
        if F(uvt_t - INF) > -PZERO and typ != 2 and not skipping:
            ray.final = (ray.color * env).astype(np.float32)
            ray.color = (ray.color * F(0.0)).astype(np.float32)
            ray.set(ACT, 0)
            skipping = True
        ray.direct = normalize(ray.direct)
        ray.origin = (ray.origin + ray.direct * uvt_t).astype(np.float32)
        if ray.get(ACT) < 1 or n == 0:
            skipping = True
        surfacenormal = normal_h
        normal = surfacenormal if dot(surfacenormal, ray.direct) < 0 else (-surfacenormal).astype(np.float32)
        refly = mr[0]
        pw = clamp(F(np.power(abs(dot(ray.direct, normal)), F(F(1.4) - F(1.0)), dtype=np.float32)), 0.0, 1.0)
        dielectric = mix(F(1.0), F(0.05), pw)
        sm = F(np.sqrt(mr[1]))
        sc = v3(*[mix(dielectric, albedo[k], sm) for k in range(3)])
        emis = mlength(emission[:3])
        spca = clamp(mlength(sc), 0.0, 1.0)
        prom = F(F(1.0) - albedo[3])
        aprom = prom if typ == 2 else (F(1.0) if g.next() < prom else F(0.0))
        diffuse_ray, reflection_ray, emissive_ray = ray.copy(), ray.copy(), ray.copy()
        for q in (diffuse_ray, reflection_ray, emissive_ray):
            q.final = (q.final * F(0.0)).astype(np.float32)
        if not skipping:
            ray.final = (ray.final * F(0.0)).astype(np.float32)
        if ray.get(ACT) > 0 and not skipping:
            # diffuse(), shadinglib.glsl:106-119 (DIRECT_LIGHT_ENABLED)
            q = diffuse_ray
            q.color = (q.color * albedo[:3]).astype(np.float32)
            q.direct = normalize(random_cosine(g, normal))
            q.origin = (q.direct * GAP + q.origin).astype(np.float32)
            q.set(ACT, 0 if q.get(TYPE) == 2 else q.get(ACT))
            q.set(BOUNCE, min(2, q.get(BOUNCE)))
            q.set(TYPE, 1)
            q.set(DL, 0)
            # reflection(), :139-148 (SUNLIGHT_CAUSTICS false)
            q = reflection_ray
            col = clamp((sc / spca).astype(np.float32), 0.0, 1.0)
            dn = dot(normal, q.direct)
            refl = (q.direct - normal * F(F(2.0) * dn)).astype(np.float32)
            rc = random_cosine(g, normal)
            al = clamp(F(refly * g.next()), 0.0, 1.0)
            q.direct = normalize(mix(refl, rc, al))
            q.color = (q.color * col).astype(np.float32)
            q.origin = (q.direct * GAP + q.origin).astype(np.float32)
            q.set(DL, 0 if q.get(TYPE) == 1 else 1)
            q.set(TYPE, 0)
            q.set(BOUNCE, min(3, q.get(BOUNCE)))
            q.set(ACT, 0 if q.get(TYPE) == 2 else q.get(ACT))
            # emissive(), :127-137
            q = emissive_ray
            q.final = np.maximum((q.color * emission[:3]).astype(np.float32), F(0.0))
            if q.get(TYPE) == 1:
                q.final = v3(0, 0, 0)
            q.color = (q.color * F(0.0)).astype(np.float32)
            q.direct = normalize(random_cosine(g, normal))
            q.origin = (q.direct * GAP + q.origin).astype(np.float32)
            q.set(BOUNCE, 0); q.set(ACT, 0); q.set(DL, 0)
            # promised(), :121-125
            ray.set(BOUNCE, ray.get(BOUNCE) + 1)
            ray.origin = (ray.direct * GAP + ray.origin).astype(np.float32)
            ray.color = (ray.color * aprom).astype(np.float32)
            ray.final = (ray.final * aprom).astype(np.float32)
        else:
            for q in (reflection_ray, emissive_ray, diffuse_ray):
                q.color = (q.color * F(0.0)).astype(np.float32)
            diffuse_ray.final = (diffuse_ray.final * F(0.0)).astype(np.float32)
        if not skipping:
            om = F(F(1.0) - aprom)
            diffuse_ray.color = (diffuse_ray.color * om).astype(np.float32)
            diffuse_ray.final = (diffuse_ray.final * om).astype(np.float32)
            reflection_ray.color = (reflection_ray.color * om).astype(np.float32)
            emissive_ray.final = (emissive_ray.final * F(om * F(F(1.0) - clamp(spca, 0.0, 1.0)))).astype(np.float32)
        if ray.get(BASIS) == 1 and aprom < F(0.1):
            ray.set(BASIS, 0)
        # reclaim the current ray (:235-251): storeRay deposits, addRayToList queues
        bounce = ray.get(BOUNCE) - 1
        # max(vec3(0.0f), v): GLSL's max(x, y) is `x < y ? y : x`, so a NaN component of v gives x = 0 -- numpy's maximum would hand the NaN
        # on and the ray would stay active with a NaN colour (round 5: the fuzzer's black full-metal surfaces,
        # tests/test_oracle_cpu.py::test_fuzzed_scenes_shade_against_the_independent_reading)
        ray.final = np.where(F(0.0) < ray.final, ray.final, F(0.0)).astype(np.float32)
        ray.color = np.where(F(0.0) < ray.color, ray.color, F(0.0)).astype(np.float32)
        if bounce < 0 or mlength(ray.color) < F(0.0001) or n == 0:
            ray.set(ACT, 0)
        ray.set(BOUNCE, bounce if bounce >= 0 else 0)
        if mlength(ray.final) >= F(0.0001) and ray.get(ACT) == 0:
            sink.collect(ray)
        if ray.get(ACT) == 1:
            sink.out.append((ray.origin.copy(), ray.direct.copy(), ray.color.copy(), ray.b, ray.texel, pkey, it))
        # emit new rays (:263-275)
        if not skipping:
            coef = clamp(F(1.0) if g.next() < spca else F(0.0), 0.0, 1.0)
            reflection_ray.color = (reflection_ray.color * coef).astype(np.float32)
            diffuse_ray.color = (diffuse_ray.color * F(F(1.0) - coef)).astype(np.float32)
            # directLight(0, diffuseRay, 1, normal), shadinglib.glsl:75-93
            sh = diffuse_ray.copy()
            sh.set(ACT, 0 if sh.get(TYPE) == 2 else sh.get(ACT))
            sh.set(DL, 1); sh.set(TYPE, 2); sh.set(TARGET, 0)
            sh.set(BOUNCE, min(1, sh.get(BOUNCE)))
            L0 = lights[0]
            ctr = light_center(L0)
            radius = F(L0["lightColor"][3])
            sl = (random_direction_in_sphere(g) * F(radius - F(0.0001)) + ctr).astype(np.float32)
            ldirect = normalize((sl - sh.origin).astype(np.float32))
            d = (ctr - sh.origin).astype(np.float32)
            dist = F(np.sqrt(dot(d, d)))
            q2 = F(np.power(F(radius / dist), F(2.0), dtype=np.float32))
            weight = F(F(1.0) - F(np.sqrt(F(F(1.0) - clamp(F(F(dot(ldirect, normal) * F(2.0)) * q2), 0.0, 1.0)))))
            sh.origin = (sh.direct * (-GAP) + sh.origin).astype(np.float32)
            sh.direct = ldirect
            sh.color = (sh.color * F(F(1.0) * weight)).astype(np.float32)
            sh.final = (sh.final * F(0.0)).astype(np.float32)
            sh.origin = (sh.direct * GAP + sh.origin).astype(np.float32)
            sink.create_ray(diffuse_ray, child_key(pkey, 1))
            sink.create_ray(reflection_ray, child_key(pkey, 2))
            ce = clamp(emis, 0.0, 1.0)
            emissive_ray.color = (emissive_ray.color * ce).astype(np.float32)
            emissive_ray.final = (emissive_ray.final * ce).astype(np.float32)
            sink.create_ray(emissive_ray, child_key(pkey, 4))
            # applyLight, shadinglib.glsl:181-189
            if diffuse_ray.get(TYPE) == 2 or dot(surfacenormal, sh.direct) < 0:
                sh.set(ACT, 0)
            sink.create_ray(sh, child_key(pkey, 3))
    flush()
    return sink.out, sink.tex
