"""Seeded random scenes in the flattened form of include/rtr_hip.h, built from the same object kinds the
reference's scene builders use (scene/scenes.cpp): spheres, moving spheres, the three rects, `box`
(geometry/box.h:18-31: six rects in a hittable_list), translate(rotate_y(box)), flip_face, nested
hittable_lists, constant_medium, QuadLights over emissive rects.  Test infrastructure: the golden scenes pin
the oracle against the reference; these scenes let the pinned oracle check the device on graphs no demo
scene contains (coplanar overlapping rects, media next to transforms, many small instances, ...)."""
import numpy as np

import _golden as G

A = G.A
rtr = G.rtr


# material palettes of random_scene: which material / texture / light classes a scene may use.  They aim at the
# material-set variants of the kernels (csrc/rt_device.h: RT_MS_*), which upload picks from what the scene holds.
#   full     every material, checker and noise textures, any light (RT_MS_FULL)
#   quadlit  every material, solid textures only, QuadLights only (RT_MS_QUADLIT: no texture reads (u,v))
#   lean     lambertian and diffuse_light with solid textures, QuadLights only (RT_MS_LEAN)
PALETTES = ("full", "quadlit", "lean")


class Builder:
    def __init__(self, rng, palette="full"):
        assert palette in PALETTES, palette
        self.rng = rng
        self.palette = palette
        self.nodes, self.kids, self.mats, self.texs, self.lights = [], [], [], [], []
        self.uses_noise = False

    # ---- records ---------------------------------------------------------------------------------
    def node(self, type_, a=0, b=0, f=()):
        n = np.zeros(1, dtype=A.NODE_DTYPE)
        n["type"], n["a"], n["b"] = type_, a, b
        n["f"][0, :len(f)] = f
        self.nodes.append(n)
        return len(self.nodes) - 1

    def solid(self, rgb):
        t = np.zeros(1, dtype=A.TEXTURE_DTYPE)
        t["type"] = A.TEX_SOLID
        t["f"][0, :3] = rgb
        self.texs.append(t)
        return len(self.texs) - 1

    def checker(self, even, odd):
        t = np.zeros(1, dtype=A.TEXTURE_DTYPE)
        t["type"], t["a"], t["b"] = A.TEX_CHECKER, even, odd
        self.texs.append(t)
        return len(self.texs) - 1

    def noise(self, scale):
        t = np.zeros(1, dtype=A.TEXTURE_DTYPE)
        t["type"], t["a"] = A.TEX_NOISE, 0  # perlin table 0 (the scene carries scene 9's)
        t["f"][0, 0] = scale
        self.texs.append(t)
        self.uses_noise = True
        return len(self.texs) - 1

    def material(self, type_, tex=(), f=()):
        m = np.zeros(1, dtype=A.MATERIAL_DTYPE)
        m["type"] = type_
        m["tex"][0, :] = -1
        m["tex"][0, :len(tex)] = tex
        if type_ not in (A.MAT_PBR,):
            m["tex"][0, len(tex):] = 0
        m["f"][0, :len(f)] = f
        self.mats.append(m)
        return len(self.mats) - 1

    # ---- materials the reference's scenes use -------------------------------------------------------
    def random_material(self, allow_glass=True):
        r = self.rng
        k = int(r.integers(0, 6 if allow_glass else 5))
        if self.palette == "lean":  # the glass draw becomes an emitter that is no QuadLight, the rest solid lambertian
            if k == 5:
                return self.material(A.MAT_DIFFUSE_LIGHT, [self.solid(r.uniform(1.0, 4.0, 3))])
            return self.material(A.MAT_LAMBERTIAN, [self.solid(r.uniform(0.1, 0.9, 3))])
        if self.palette == "quadlit" and k in (0, 1):  # no checker, no noise
            return self.material(A.MAT_LAMBERTIAN, [self.solid(r.uniform(0.1, 0.9, 3))])
        if k == 0 and r.random() < 0.3:  # marble-like noise_texture (texture.h:78-92)
            return self.material(A.MAT_LAMBERTIAN, [self.noise(float(r.uniform(0.5, 6.0)))])
        if k == 0:
            return self.material(A.MAT_LAMBERTIAN, [self.solid(r.uniform(0.1, 0.9, 3))])
        if k == 1:
            return self.material(A.MAT_LAMBERTIAN, [self.checker(self.solid(r.uniform(0.1, 0.4, 3)),
                                                                 self.solid(r.uniform(0.6, 0.9, 3)))])
        if k == 2:
            return self.material(A.MAT_METAL, f=list(r.uniform(0.5, 0.95, 3)) + [float(r.choice([0.0, 0.1, 0.5]))])
        if k in (3, 4):
            rough, metal = float(r.choice([0.01, 0.05, 0.2, 0.4, 1.0])), float(r.choice([0.0, 0.5, 1.0]))
            return self.material(A.MAT_PBR, [self.solid(r.uniform(0.2, 0.9, 3)), self.solid([rough] * 3),
                                             self.solid([metal] * 3), -1])
        return self.material(A.MAT_DIELECTRIC, f=[1.5])

    # ---- geometry ----------------------------------------------------------------------------------------
    def sphere(self, c, radius, mat):
        return self.node(A.NODE_SPHERE, mat, f=list(c) + [radius])

    def moving_sphere(self, c0, c1, radius, mat):
        return self.node(A.NODE_MOVING_SPHERE, mat, f=list(c0) + list(c1) + [0.0, 1.0, radius])

    def rect(self, axis, a0, a1, b0, b1, k, mat):
        return self.node({"xy": A.NODE_XY_RECT, "xz": A.NODE_XZ_RECT, "yz": A.NODE_YZ_RECT}[axis], mat, f=[a0, a1, b0, b1, k])

    def hlist(self, children):
        first = len(self.kids)
        self.kids += list(children)
        return self.node(A.NODE_LIST, first, len(children))

    def box(self, p0, p1, mat):
        """geometry/box.h:18-31, the order of its six sides"""
        s = [self.rect("xy", p0[0], p1[0], p0[1], p1[1], p1[2], mat), self.rect("xy", p0[0], p1[0], p0[1], p1[1], p0[2], mat),
             self.rect("xz", p0[0], p1[0], p0[2], p1[2], p1[1], mat), self.rect("xz", p0[0], p1[0], p0[2], p1[2], p0[1], mat),
             self.rect("yz", p0[1], p1[1], p0[2], p1[2], p1[0], mat), self.rect("yz", p0[1], p1[1], p0[2], p1[2], p0[0], mat)]
        return self.hlist(s)

    def translate(self, child, off):
        return self.node(A.NODE_TRANSLATE, child, f=list(off))

    def rotate_y(self, child, degrees):
        rad = degrees * np.pi / 180.0  # hittable.h:98-100 (degrees_to_radians, then sin / cos)
        return self.node(A.NODE_ROTATE_Y, child, f=[np.sin(rad), np.cos(rad)])

    def flip_face(self, child):
        return self.node(A.NODE_FLIP_FACE, child)

    def medium(self, boundary, density, rgb):
        phase = self.material(A.MAT_ISOTROPIC, [self.solid(rgb)])
        return self.node(A.NODE_MEDIUM, boundary, phase, f=[-1.0 / density])

    def quad_light(self, q, u, v, intensity):
        n = np.cross(u, v)
        area = float(np.linalg.norm(n))
        l = np.zeros(1, dtype=A.LIGHT_DTYPE)
        l["type"] = A.LIGHT_QUAD
        l["f"][0, :] = list(q) + list(u) + list(v) + list(intensity) + list(n / area) + [area]
        self.lights.append(l)


    def simple_light(self, type_, f):
        l = np.zeros(1, dtype=A.LIGHT_DTYPE)
        l["type"] = type_
        l["f"][0, :len(f)] = f
        self.lights.append(l)


def _cat(parts, dtype):
    return np.concatenate(parts) if parts else np.zeros(0, dtype=dtype)


def random_scene(seed, n_objects=24, media=False, hollow=False, ties=True, delta_lights=False, lens=0.0, moved_media=False,
                 big_group=False, palette="full", hollow_pairs=0, bare_hollows=0, hollow_lists=0, spheres_only=False):
    """One scene in front of scene 23's camera (origin (0,3,8), looking at the origin).  `palette` (PALETTES): the
    material and light classes it may use; "full" draws exactly what this generator always drew, so every seed of
    the default palette gives the same scene, byte for byte, as before palettes existed.
    Several hollow spheres (negative radius: an inverted bounding box, so the bvh_node boxes above one do not enclose
    it), all off by default and drawn after everything else, so the scenes without them stay as they were:
      hollow_pairs   that many more hollow-in-glass pairs like `hollow`'s
      bare_hollows   that many hollow spheres on their own
      hollow_lists   that many nested hittable_lists of 2-4 bare hollow spheres each (under a bvh_node, no box is
                     entered between two of them, so an earlier one's hit can shrink t_max below the boxes above both)
      spheres_only   the n_objects drawn are solid spheres only (no transforms, no rects beyond ground and light), so a
                     scene with hollow spheres stays one linearly scanned instance (the guarded references)"""
    if delta_lights and palette != "full":
        raise ValueError("palette %r has QuadLights only" % palette)
    rng = np.random.default_rng(seed)
    b = Builder(rng, palette)
    base = G.scene(23)
    top = []
    if palette == "full":
        ground = b.material(A.MAT_LAMBERTIAN, [b.checker(b.solid([0.2, 0.3, 0.1]), b.solid([0.9, 0.9, 0.9]))])
    else:
        ground = b.material(A.MAT_LAMBERTIAN, [b.solid([0.45, 0.5, 0.35])])
    # (not at y = 0: there sin(10 * p.y) of the checker would be the sign of the hit point's rounding noise, and a
    # last-bit difference between two libms upstream of the hit would flip whole checker cells)
    top.append(b.rect("xz", -12.0, 12.0, -12.0, 12.0, -0.013, ground))
    # an area light: emissive rect facing down behind a flip_face (scenes.cpp:779-809) + its QuadLight
    emit = b.material(A.MAT_DIFFUSE_LIGHT, [b.solid([7.0, 7.0, 7.0])])
    lx0, lx1, lz0, lz1, ly = -2.0, 2.0, -3.0, 0.0, 6.0
    top.append(b.flip_face(b.rect("xz", lx0, lx1, lz0, lz1, ly, emit)))
    b.quad_light([lx0, ly, lz0], [lx1 - lx0, 0.0, 0.0], [0.0, 0.0, lz1 - lz0], [7.0, 7.0, 7.0])

    if delta_lights:  # lighting/point_light.h, spot_light.h, directional_light.h, environmental_light.h without a map
        b.simple_light(A.LIGHT_POINT, [3.0, 4.5, 1.0, 9.0, 8.0, 6.0])
        d = np.array([-0.3, -1.0, -0.2])
        b.simple_light(A.LIGHT_SPOT, [-3.0, 5.0, 0.0] + list(d / np.linalg.norm(d)) + [20.0, 20.0, 25.0, np.cos(np.radians(35.0))])
        d = np.array([0.4, -1.0, 0.3])
        b.simple_light(A.LIGHT_DIRECTIONAL, list(d / np.linalg.norm(d)) + [0.6, 0.5, 0.4])
        b.simple_light(A.LIGHT_ENV_UNIFORM, [])

    def pos(lo=(-4.5, 0.3, -6.0), hi=(4.5, 3.5, 2.0)):
        return rng.uniform(lo, hi)

    for _ in range(n_objects):
        kind = int(rng.integers(0, 8)) if not spheres_only else 0
        mat = b.random_material()
        if kind == 0:
            top.append(b.sphere(pos(), float(rng.uniform(0.15, 0.7)), mat))
        elif kind == 1:
            c = pos()
            top.append(b.moving_sphere(c, c + rng.uniform(-0.3, 0.3, 3), float(rng.uniform(0.15, 0.5)), mat))
        elif kind == 2:
            axis = ["xy", "xz", "yz"][int(rng.integers(0, 3))]
            a0, b0 = rng.uniform(-4.0, 3.0, 2)
            k = float(rng.uniform(-5.0, 3.0)) if axis != "xz" else float(rng.uniform(0.2, 3.0))
            r1 = b.rect(axis, a0, a0 + rng.uniform(0.3, 2.0), b0, b0 + rng.uniform(0.3, 2.0), k, mat)
            top.append(r1)
            if ties and rng.random() < 0.5:
                # a second rect in the SAME plane that overlaps the first one, other material: exact ties in t,
                # the reference keeps the one its hittable_list visits later (aarect.h accepts t == t_max)
                n1 = b.nodes[r1]["f"][0]
                top.append(b.rect(axis, n1[0] + 0.1, n1[1] + 0.4, n1[2] - 0.2, n1[3] - 0.05, k, b.random_material(False)))
        elif kind == 3:
            p0 = pos()
            top.append(b.box(p0, p0 + rng.uniform(0.2, 1.2, 3), mat))
        elif kind in (4, 5):
            size = rng.uniform(0.3, 1.3, 3)
            inner = b.box([0.0, 0.0, 0.0], size, mat)
            top.append(b.translate(b.rotate_y(inner, float(rng.uniform(-60.0, 60.0))), pos()))
        elif kind == 6:
            # a small group of its own (nested hittable_list), partly under a translate
            grp = [b.sphere(rng.uniform(-0.5, 0.5, 3), float(rng.uniform(0.1, 0.3)), b.random_material()) for _ in range(3)]
            top.append(b.translate(b.hlist(grp), pos()))
        else:
            top.append(b.flip_face(b.sphere(pos(), float(rng.uniform(0.2, 0.5)), mat)))
    if big_group:
        # dozens of primitives under ONE transform chain (scenes.cpp:278-287: translate(rotate_y(bvh_node(boxes2)))): an
        # instance with a box tree of its own, which a top tree over the instances walks nested on the same stack
        grp = [b.sphere(rng.uniform(-1.2, 1.2, 3), float(rng.uniform(0.08, 0.25)), b.random_material()) for _ in range(40)]
        grp += [b.box(p0, p0 + rng.uniform(0.15, 0.5, 3), b.random_material()) for p0 in rng.uniform(-1.2, 1.0, (6, 3))]
        top.append(b.translate(b.rotate_y(b.hlist(grp), float(rng.uniform(-40.0, 40.0))), pos((-3.0, 1.2, -4.0), (3.0, 2.5, 0.0))))
    if hollow:  # hollow glass (scenes.cpp:903): negative radius inside a glass sphere (lean palette: a lambertian shell)
        c = pos()
        if palette == "lean":
            glass = b.material(A.MAT_LAMBERTIAN, [b.solid([0.8, 0.6, 0.3])])
        else:
            glass = b.material(A.MAT_DIELECTRIC, f=[1.5])
        top.append(b.sphere(c, 0.6, glass))
        top.append(b.sphere(c, -0.5, glass))
    for _ in range(hollow_pairs):
        c, r = pos(), float(rng.uniform(0.4, 0.8))
        glass = b.material(A.MAT_DIELECTRIC, f=[1.5]) if palette != "lean" else b.random_material()
        top.append(b.sphere(c, r, glass))
        top.append(b.sphere(c, -0.85 * r, glass))
    for _ in range(bare_hollows):
        top.append(b.sphere(pos(), -float(rng.uniform(0.2, 0.6)), b.random_material()))
    for _ in range(hollow_lists):
        c = pos()
        members = [b.sphere(c + rng.uniform(-1.0, 1.0, 3), -float(rng.uniform(0.2, 0.6)), b.random_material())
                   for _ in range(int(rng.integers(2, 5)))]
        top.insert(int(rng.integers(0, len(top) + 1)), b.hlist(members))
    if media:
        c = pos()
        shell = ground if palette == "lean" else b.material(A.MAT_DIELECTRIC, f=[1.5])
        top.append(b.medium(b.sphere(c, 0.9, shell), 0.8, [0.2, 0.4, 0.9]))
        p0 = pos()
        top.append(b.medium(b.box(p0, p0 + rng.uniform(0.6, 1.5, 3), ground), 1.5, [0.9, 0.9, 0.9]))
        top.append(b.medium(b.sphere([0.0, 0.0, 0.0], 40.0, ground), 0.01, [1.0, 1.0, 1.0]))  # mist around everything
        order = rng.permutation(len(top))  # media anywhere in the visiting order, not only at its end
        top = [top[i] for i in order]
    if moved_media:  # a medium UNDER a transform (scenes.cpp:214-217: cornell_smoke's boxes): no step program for it
        smoke = b.medium(b.box([0.0, 0.0, 0.0], [1.2, 1.6, 1.1], ground), 1.2, [0.1, 0.1, 0.1])
        top.insert(len(top) // 2, b.translate(b.rotate_y(smoke, 25.0), pos()))
        top.insert(len(top) // 3, b.translate(b.medium(b.sphere([0.0, 0.0, 0.0], 0.8, ground), 2.0, [0.9, 0.8, 0.7]), pos()))
    root = b.hlist(top)
    camera = base.camera.copy()
    camera["lens_radius"] = lens  # camera.h:33-39: the defocus disk is drawn for every ray, used when the lens is open
    sc = rtr.Scene(root, _cat(b.nodes, A.NODE_DTYPE), np.asarray(b.kids, dtype=np.int32), _cat(b.mats, A.MATERIAL_DTYPE),
                   _cat(b.texs, A.TEXTURE_DTYPE), G.scene(9).perlin[:1] if b.uses_noise else base.perlin[:0],
                   base.images[:0], base.image_bytes[:0],
                   _cat(b.lights, A.LIGHT_DTYPE), camera, np.array([0.55, 0.65, 0.8]))
    return sc


def single_type_scene(seed, kind="metal", light="quad", n_objects=10):
    """A scene whose materials are all of ONE type, so the wavefront pipeline shades it without sorting by material
    class (WavefrontPlan::sort needs two types; every random_scene has at least lambertian + diffuse_light).
      kind   "metal": metal spheres and boxes; "fog": constant_media whose boundaries carry the phase material too
             (a scene with media shades in two phases where it has lights)
      light  "quad": one QuadLight (RT_MS_QUADLIT where no texture reads (u,v)); "point": a point light (RT_MS_FULL)
    The lights sit in the light list only: nothing in the graph emits, the light sampling alone reaches them."""
    rng = np.random.default_rng(seed)
    b = Builder(rng)
    base = G.scene(23)
    top = []
    if kind == "metal":
        for _ in range(n_objects):
            mat = b.material(A.MAT_METAL, f=list(rng.uniform(0.5, 0.95, 3)) + [float(rng.choice([0.0, 0.1, 0.5]))])
            p0 = rng.uniform((-4.5, 0.3, -6.0), (4.5, 3.5, 2.0))
            if rng.random() < 0.5:
                top.append(b.sphere(p0, float(rng.uniform(0.2, 0.8)), mat))
            else:
                top.append(b.box(p0, p0 + rng.uniform(0.3, 1.2, 3), mat))
        top.append(b.rect("xz", -12.0, 12.0, -12.0, 12.0, -0.013, b.material(A.MAT_METAL, f=[0.7, 0.7, 0.7, 0.3])))
    else:
        assert kind == "fog", kind
        for _ in range(n_objects):
            phase = b.material(A.MAT_ISOTROPIC, [b.solid(rng.uniform(0.2, 0.9, 3))])
            p0 = rng.uniform((-4.5, 0.3, -6.0), (4.5, 3.5, 2.0))
            if rng.random() < 0.5:
                boundary = b.sphere(p0, float(rng.uniform(0.4, 1.0)), phase)
            else:
                boundary = b.box(p0, p0 + rng.uniform(0.5, 1.5, 3), phase)
            top.append(b.node(A.NODE_MEDIUM, boundary, phase, f=[-1.0 / float(rng.uniform(0.3, 3.0))]))
    if light == "quad":
        b.quad_light([-2.0, 6.0, -3.0], [4.0, 0.0, 0.0], [0.0, 0.0, 3.0], [7.0, 7.0, 7.0])
    else:
        assert light == "point", light
        b.simple_light(A.LIGHT_POINT, [1.0, 5.0, -1.0, 30.0, 28.0, 25.0])
    root = b.hlist(top)
    return rtr.Scene(root, _cat(b.nodes, A.NODE_DTYPE), np.asarray(b.kids, dtype=np.int32), _cat(b.mats, A.MATERIAL_DTYPE),
                     _cat(b.texs, A.TEXTURE_DTYPE), base.perlin[:0], base.images[:0], base.image_bytes[:0],
                     _cat(b.lights, A.LIGHT_DTYPE), base.camera.copy(), np.array([0.55, 0.65, 0.8]))


def random_rays(seed, n):
    rng = np.random.default_rng(seed)
    rays = np.zeros(n, dtype=A.HIT_DTYPE)
    rays["o"] = rng.uniform((-6.0, 0.2, -7.0), (6.0, 6.0, 8.0), (n, 3))
    target = rng.uniform((-4.5, 0.0, -6.0), (4.5, 3.5, 2.0), (n, 3))
    rays["d"] = target - rays["o"]
    rays["time"] = rng.uniform(0.0, 1.0, n)
    rays["t_min"], rays["t_max"] = 0.001, np.inf
    rays["rng_in"] = rng.integers(1, 2 ** 32 - 1, n, dtype=np.uint64).astype(np.uint32)
    return rays


def cross_instance_tie_scene():
    """Exact ties in t between objects under DIFFERENT transform chains: faces of translated (and rotated) boxes in
    the planes of rects that the list visits before and after them.  The reference keeps whatever it visits later."""
    b = Builder(np.random.default_rng(0))
    m = [b.material(A.MAT_LAMBERTIAN, [b.solid(c)]) for c in ([.9, .1, .1], [.1, .9, .1], [.1, .1, .9], [.9, .9, .1],
                                                             [.1, .9, .9], [.9, .1, .9], [.5, .5, .5])]
    floor_a = b.rect("xz", -5, 5, -5, 5, 0.0, m[0])
    back = b.rect("xy", -5, 5, -1, 4, 1.5, m[5])
    t1 = b.translate(b.rotate_y(b.box([0, 0, 0], [1, 1.5, 1], m[1]), 20.0), [0.5, 0.0, -1.0])  # bottom in y = 0
    floor_b = b.rect("xz", -1, 3, -3, 1, 0.0, m[2])  # same transform chain as floor_a, visited AFTER t1
    t2 = b.translate(b.box([0, 0, 0], [1, 1, 1], m[3]), [-2.0, 0.0, 0.5])  # faces in x = -2, z = 1.5, y = 0
    side = b.rect("yz", -1, 4, -5, 5, -2.0, m[4])  # visited after t2
    t3 = b.translate(b.translate(b.box([0, 0, 0], [0.5, 0.5, 0.5], m[6]), [1.0, 0.0, 0.0]), [1.5, 0.0, 1.0])  # z = 1.5 again
    root = b.hlist([floor_a, back, t1, floor_b, t2, side, t3])
    base = G.scene(23)
    return rtr.Scene(root, _cat(b.nodes, A.NODE_DTYPE), np.asarray(b.kids, dtype=np.int32), _cat(b.mats, A.MATERIAL_DTYPE),
                     _cat(b.texs, A.TEXTURE_DTYPE), base.perlin[:0], base.images[:0], base.image_bytes[:0], base.lights[:0],
                     base.camera.copy(), np.array([0.5, 0.6, 0.8]))


def cross_instance_tie_rays(n=1536):
    rng = np.random.default_rng(5)
    r = np.zeros(n, dtype=A.HIT_DTYPE)
    k = n // 3
    o, t = np.empty((n, 3)), np.empty((n, 3))
    o[:k] = rng.uniform((-3, -3, -3), (3.5, -0.5, 3), (k, 3))  # from below the floors, up into the boxes
    t[:k] = rng.uniform((-2.2, 0.2, -1.2), (3.2, 1.2, 1.8), (k, 3))
    o[k:2 * k] = rng.uniform((-6, 0.1, -1), (-2.5, 2, 3), (k, 3))  # from x < -2 into the translated box
    t[k:2 * k] = rng.uniform((-1.9, 0.1, 0.6), (-1.1, 0.9, 1.4), (k, 3))
    o[2 * k:] = rng.uniform((-3, 0.1, 2), (4, 2, 5), (n - 2 * k, 3))  # from z > 1.5
    t[2 * k:] = rng.uniform((-1.9, 0.05, 0.6), (3.0, 0.9, 1.45), (n - 2 * k, 3))
    r["o"], r["d"] = o, t - o
    r["time"], r["t_min"], r["t_max"], r["rng_in"] = 0.5, 0.001, np.inf, 7
    return r


# ---- several hollow spheres under bvh_nodes ---------------------------------------------------------------------------
_PAD = 0.0001  # aarect.h: kAABBPadding around a rect's plane


def _node_box(sc, ix):
    """bounding_box of the reference's classes for the node kinds of spheres_only scenes (sphere.h:62-66: a negative
    radius gives an inverted box; aarect.h; hittable_list.h:49-62 and aabb.h:50-59: surrounding boxes; flip_face)"""
    n = sc.nodes[ix]
    t, f = int(n["type"]), n["f"]
    if t == A.NODE_SPHERE:
        c, r = np.array(f[:3]), float(f[3])
        return c - r, c + r
    if t in (A.NODE_XY_RECT, A.NODE_XZ_RECT, A.NODE_YZ_RECT):
        k = {A.NODE_XY_RECT: 2, A.NODE_XZ_RECT: 1, A.NODE_YZ_RECT: 0}[t]
        a, b_ = [ax for ax in range(3) if ax != k]
        lo, hi = np.empty(3), np.empty(3)
        lo[a], hi[a], lo[b_], hi[b_] = f[0], f[1], f[2], f[3]
        lo[k], hi[k] = f[4] - _PAD, f[4] + _PAD
        return lo, hi
    if t == A.NODE_FLIP_FACE:
        return _node_box(sc, int(n["a"]))
    if t == A.NODE_LIST:
        boxes = [_node_box(sc, int(sc.list_children[int(n["a"]) + k])) for k in range(int(n["b"]))]
        return np.min([b_[0] for b_ in boxes], axis=0), np.max([b_[1] for b_ in boxes], axis=0)
    raise ValueError("bvh_over_top: no box rule for node type %d" % t)


def bvh_over_top(sc, seed):
    """The scene with its root hittable_list replaced by a tree of bvh_nodes over the list's objects, built the way
    bvh_node's constructor builds one (bvh.h:53-96: a random split axis per node, objects sorted by their boxes'
    minimum on it, one object -> left = right = it, two -> in comparator order, more -> halves).  The axes come from
    numpy, not from the reference's RNG, so this is not the tree `wrap-bvh` builds -- it needs no reference to run,
    and the oracle answers for it.  Node kinds: those of spheres_only scenes."""
    rng = np.random.default_rng(seed)
    nodes = list(sc.nodes)
    root = sc.nodes[sc.root]
    assert int(root["type"]) == A.NODE_LIST
    objs = [int(sc.list_children[int(root["a"]) + k]) for k in range(int(root["b"]))]
    box = {ix: _node_box(sc, ix) for ix in objs}

    def build(items):
        axis = int(rng.integers(0, 3))
        if len(items) == 1:
            left = right = items[0]
        elif len(items) == 2:
            left, right = items if box[items[0]][0][axis] < box[items[1]][0][axis] else items[::-1]
        else:
            items = sorted(items, key=lambda ix: box[ix][0][axis])  # (stable, like std::sort on distinct keys)
            mid = len(items) // 2
            left, right = build(items[:mid]), build(items[mid:])
        n = np.zeros(1, dtype=A.NODE_DTYPE)
        n["type"], n["a"], n["b"] = A.NODE_BVH, left, right
        lo = np.minimum(box[left][0], box[right][0])
        hi = np.maximum(box[left][1], box[right][1])
        n["f"][0, :6] = list(lo) + list(hi)
        nodes.append(n[0])
        me = len(nodes) - 1
        box[me] = (lo, hi)
        return me

    top = build(objs)
    return rtr.Scene(top, np.array(nodes, dtype=A.NODE_DTYPE), sc.list_children, sc.materials, sc.textures, sc.perlin,
                     sc.images, sc.image_bytes, sc.lights, sc.camera, sc.background)


def guard_rule_split(sc, rays):
    """Indices of the rays on which the device's former guard rule (oracle rto_hits_running_guard: every bvh_node box
    above a hollow sphere tested with the running t_max) and the reference's walk (rto_hits: each box with the t_max
    its node was entered with) give different hit records."""
    ref = G.oracle_records(sc, "rto_hits", rays)
    run = G.oracle_records(sc, "rto_hits_running_guard", rays)
    return np.flatnonzero((ref["hit"] != run["hit"]) | (ref["material"] != run["material"]) |
                          (ref["t"].view(np.uint64) != run["t"].view(np.uint64)))


def discriminating_rays(sc, seed, n, pool=65536, most=None):
    """`n` rays: those of `pool` candidates (random_rays(100000 + seed, pool)) on which the two guard rules disagree --
    at most `most` of them, n // 2 by default --, topped up with random_rays(seed, ...) in their usual order."""
    cand = random_rays(100000 + seed, pool)
    pick = cand[guard_rule_split(sc, cand)[:n // 2 if most is None else most]]
    return np.concatenate([pick, random_rays(seed, n - len(pick))])
