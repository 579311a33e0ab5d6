"""Small flat scenes for the finish records of the flat kernels (csrc/rt_device.h: struct FFin), and the reference's walk over
a scene restated in Python: which primitive the reference visits at which position, under which wrappers.

A synthetic scene is a room (one large sphere in the world frame) around four clusters, one per transform chain: none, T, R
and one chain of two levels, T(R(.)) or R(T(.)).  A cluster is a box whose six sides carry six materials and a sphere.
``flips`` is a mask over the three places a flip_face can sit in a chain -- bit 0 outside the outermost transform, bit 1
between the levels (on a chain of one level: inside it), bit 2 innermost, around the cluster -- and the sphere always carries
one flip_face more than the box, so a set bit 2 gives it two in a row."""
import numpy as np

import _golden as G
import _randscene as R

A = G.A
rtr = G.rtr
BASE = G.scene(23)  # camera and empty arrays

BOX_P0, BOX_P1 = np.array([-0.8, -0.7, -0.9]), np.array([0.9, 0.8, 0.7])
SPHERE_C, SPHERE_R = np.array([0.2, 2.0, 0.1]), 0.6
CHAINS = ("none", "T", "R", "two")
SIDES_PER_CLUSTER = 7  # six box sides + the sphere: materials 7 * chain + side


def _scene(b, top):
    root = b.hlist(top)
    return rtr.Scene(root, R._cat(b.nodes, A.NODE_DTYPE), np.asarray(b.kids, dtype=np.int32), R._cat(b.mats, A.MATERIAL_DTYPE),
                     R._cat(b.texs, A.TEXTURE_DTYPE), BASE.perlin[:0], BASE.images[:0], BASE.image_bytes[:0],
                     R._cat(b.lights, A.LIGHT_DTYPE), BASE.camera.copy(), np.array([0.5, 0.6, 0.8]))


def _grey(b, v=0.5):
    return b.material(A.MAT_LAMBERTIAN, [b.solid([v, v, v])])


def _cluster(b, off, flip_inner):
    """box (six materials, box.h's order of sides) + sphere, moved by ``off`` in their own frame"""
    m = [_grey(b, 0.1 + 0.1 * k) for k in range(SIDES_PER_CLUSTER)]
    p0, p1 = BOX_P0 + off, BOX_P1 + off
    sides = [b.rect("xy", p0[0], p1[0], p0[1], p1[1], p1[2], m[0]), b.rect("xy", p0[0], p1[0], p0[1], p1[1], p0[2], m[1]),
             b.rect("xz", p0[0], p1[0], p0[2], p1[2], p1[1], m[2]), b.rect("xz", p0[0], p1[0], p0[2], p1[2], p0[1], m[3]),
             b.rect("yz", p0[1], p1[1], p0[2], p1[2], p1[0], m[4]), b.rect("yz", p0[1], p1[1], p0[2], p1[2], p0[0], m[5])]
    node = b.hlist([b.hlist(sides), b.flip_face(b.sphere(SPHERE_C + off, SPHERE_R, m[6]))])
    return b.flip_face(node) if flip_inner else node


# (chain as a list of ("T", offset) / ("R", degrees), outermost first; the cluster's own offset)
def chain_of(name, two):
    return {"none": ([], np.array([4.0, -1.0, 4.0])), "T": ([("T", (-4.0, 1.5, 3.5))], np.zeros(3)),
            "R": ([("R", 100.0)], np.array([5.0, 0.3, 0.0])),
            "two": ([("T", (-3.5, -2.0, -4.0)), ("R", 35.0)] if two == "TR" else [("R", 200.0), ("T", (4.5, -2.5, 0.5))],
                    np.zeros(3))}[name]


def flat_scene(flips, two="TR", light=True, extra=None):
    """-> Scene.  ``extra``: None, "three" (a cluster under three transforms: no finish records) or "moving" (a moving
    sphere in the world frame: none either)."""
    b = R.Builder(np.random.default_rng(0))
    room = _grey(b, 0.9)
    # (one sphere, not six walls: an instance of more than twelve references would get a box tree, and the scene would
    # no longer be flat)
    top = [b.sphere([0.0, 0.0, 0.0], 14.0, room)]
    room_mat = room
    for name in CHAINS:
        chain, off = chain_of(name, two)
        node = _cluster(b, off, bool(flips & 4))
        if len(chain) == 1 and (flips & 2):
            node = b.flip_face(node)  # a chain of one level has no place between levels: bit 1 sits inside it
        for depth, (kind, arg) in enumerate(reversed(chain)):  # innermost transform first
            node = b.translate(node, arg) if kind == "T" else b.rotate_y(node, arg)
            if len(chain) == 2 and depth == 0 and (flips & 2):
                node = b.flip_face(node)  # between the two levels
        if flips & 1:
            node = b.flip_face(node)
        top.append(node)
    if extra == "three":
        node = _cluster(b, np.zeros(3), False)
        top.append(b.translate(b.rotate_y(b.translate(node, (0.5, 0.0, 0.0)), 20.0), (0.0, 5.0, 0.0)))
    if extra == "moving":
        top.append(b.moving_sphere([0.0, 5.0, 0.0], [0.0, 5.5, 0.0], 0.5, room))
    if light:
        b.quad_light([-2.0, 9.0, -3.0], [4.0, 0.0, 0.0], [0.0, 0.0, 3.0], [7.0, 7.0, 7.0])
    sc = _scene(b, top)
    sc.room_material = room_mat
    return sc


SHELL_C, SHELL_R, HOLLOW_R = np.array([-3.0, 1.0, -2.0]), 1.5, -1.2


def guarded_scene():
    """A flat scene with a guarded reference (RT_TRAV_FLAT_GUARD): the room, one cluster with flip_faces and a glass
    shell -- sphere(c, 1.5) around flip_face(sphere(c, -1.2)), whose inverted box the bvh_nodes above it do not enclose
    -- under a bvh like bvh_node's.  Guarded scenes compile only where everything stands in the world frame (rt_compile.h:
    guard mode), so its finish records have no level."""
    b = R.Builder(np.random.default_rng(0))
    top = [b.sphere([0.0, 0.0, 0.0], 14.0, _grey(b, 0.9)), _cluster(b, chain_of("none", "TR")[1], True)]
    glass = b.material(A.MAT_DIELECTRIC, f=[1.5])
    inner = b.material(A.MAT_DIELECTRIC, f=[1.3])
    top += [b.sphere(SHELL_C, SHELL_R, glass), b.flip_face(b.sphere(SHELL_C, HOLLOW_R, inner))]
    b.quad_light([-2.0, 9.0, -3.0], [4.0, 0.0, 0.0], [0.0, 0.0, 3.0], [7.0, 7.0, 7.0])
    return R.bvh_over_top(_scene(b, top), 1)


def guarded_rays(seed=0):
    """random rays from the middle of the room, rays at the shell from outside, and rays from inside the shell's wall and
    from inside the hollow (those meet the hollow sphere's surface)"""
    rng = np.random.default_rng(seed)
    n = 512
    o, d = [rng.uniform(-1.0, 1.0, (n, 3))], [rng.normal(size=(n, 3))]
    src = SHELL_C + 3.0 * np.array([_unit(v) for v in rng.normal(size=(n, 3))])
    o.append(src), d.append(SHELL_C + rng.uniform(-1.0, 1.0, (n, 3)) - src)
    wall = SHELL_C + 1.35 * np.array([_unit(v) for v in rng.normal(size=(n, 3))])
    o.append(wall), d.append(rng.normal(size=(n, 3)))
    o.append(SHELL_C + rng.uniform(-0.5, 0.5, (n, 3))), d.append(rng.normal(size=(n, 3)))
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    o.append(np.tile(SHELL_C, (6, 1))), d.append(axes)
    return np.concatenate(o), np.concatenate(d)


def to_world(chain, p):
    """a point of a cluster's frame in the world frame (float arithmetic of numpy: for aiming rays only)"""
    p = np.array(p, dtype=np.float64)
    for kind, arg in reversed(chain):
        if kind == "T":
            p = p + np.array(arg)
        else:
            rad = arg * np.pi / 180.0
            s, c = np.sin(rad), np.cos(rad)
            p = np.array([c * p[0] + s * p[2], p[1], -s * p[0] + c * p[2]])
    return p


# ---- the reference's walk ------------------------------------------------------------------------------------------------
def reference_visits(sc):
    """[(primitive node, wrappers above it outermost first)] in the order hittable_list::hit / bvh_node::hit visit the
    primitives (list members in order; left, then right unless it is the same object)."""
    out = []

    def walk(ix, wrappers):
        n = sc.nodes[ix]
        t = int(n["type"])
        if t == A.NODE_LIST:
            for k in range(int(n["b"])):
                walk(int(sc.list_children[int(n["a"]) + k]), wrappers)
        elif t == A.NODE_BVH:
            walk(int(n["a"]), wrappers)
            if int(n["b"]) != int(n["a"]):
                walk(int(n["b"]), wrappers)
        elif t in (A.NODE_TRANSLATE, A.NODE_ROTATE_Y, A.NODE_FLIP_FACE):
            walk(int(n["a"]), wrappers + [ix])
        else:
            out.append((ix, wrappers))

    walk(int(sc.root), [])
    return out


# ---- rays ----------------------------------------------------------------------------------------------------------------
def rays_for(sc, two, seed=0):
    """-> (origins (n, 3), directions (n, 3), {class name: slice}).  Every ray starts inside the room, so every ray hits."""
    rng = np.random.default_rng(seed)
    o, d, classes = [], [], {}

    def add(name, oo, dd):
        oo, dd = np.atleast_2d(oo), np.atleast_2d(dd)
        first = sum(len(x) for x in o)
        o.append(oo), d.append(dd)
        classes[name] = slice(first, first + len(oo))

    n = 1024
    add("random", rng.uniform(-1.0, 1.0, (n, 3)), rng.normal(size=(n, 3)))
    axes = np.concatenate([np.eye(3), -np.eye(3)])  # (-0.0 components in the negative ones)
    add("axis", rng.uniform(-6.0, 6.0, (384, 3)), np.tile(axes, (64, 1)))
    # one or two components +0 / -0
    dz = rng.normal(size=(384, 3))
    for k in range(len(dz)):
        zero = [k % 3] if k % 2 else [k % 3, (k + 1) % 3]
        for a in zero:
            dz[k, a] = 0.0 if (k // 3) % 2 else -0.0
    add("zeros", rng.uniform(-6.0, 6.0, (384, 3)), dz)
    corners = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float64)
    edges = np.array([[0.5, y, z] for y in (0, 1) for z in (0, 1)] + [[x, 0.5, z] for x in (0, 1) for z in (0, 1)] +
                     [[x, y, 0.5] for x in (0, 1) for y in (0, 1)])
    faces = [((0.5, 0.5, 1.0), (0, 0, 1)), ((0.5, 0.5, 0.0), (0, 0, -1)), ((0.5, 1.0, 0.5), (0, 1, 0)),
             ((0.5, 0.0, 0.5), (0, -1, 0)), ((1.0, 0.5, 0.5), (1, 0, 0)), ((0.0, 0.5, 0.5), (-1, 0, 0))]
    inside_o, inside_d, aim_o, aim_d, side_o, side_d, sph_o, sph_d = [], [], [], [], [], [], [], []
    for name in CHAINS:
        chain, off = chain_of(name, two)
        p0, p1 = BOX_P0 + off, BOX_P1 + off
        centre = to_world(chain, 0.5 * (p0 + p1))
        for _ in range(48):
            inside_o.append(centre + rng.uniform(-0.3, 0.3, 3)), inside_d.append(rng.normal(size=3))
        for _ in range(6):  # from inside along the world axes, signed zeros included
            inside_o.append(centre), inside_d.append(axes[_])
        for target in np.concatenate([corners, edges]):
            w = to_world(chain, p0 + target * (p1 - p0))
            for _ in range(4):
                src = rng.uniform(-1.0, 1.0, 3)
                aim_o.append(src), aim_d.append(w - src)
        for (fc, nrm) in faces:
            fc, nrm = np.array(fc), np.array(nrm, dtype=np.float64)
            for _ in range(8):
                jitter = rng.uniform(-0.3, 0.3, 3) * (1.0 - np.abs(nrm))
                target = to_world(chain, p0 + fc * (p1 - p0) + jitter)
                src = to_world(chain, p0 + fc * (p1 - p0) + 0.5 * nrm)
                side_o.append(src), side_d.append(target - src)
        sc_w = to_world(chain, SPHERE_C + off)
        for _ in range(32):  # at the sphere from outside, and from inside it
            src = sc_w + 1.5 * _unit(rng.normal(size=3))
            sph_o.append(src), sph_d.append(sc_w + rng.uniform(-0.4, 0.4, 3) - src)
        for _ in range(8):
            sph_o.append(sc_w + rng.uniform(-0.2, 0.2, 3)), sph_d.append(rng.normal(size=3))
    add("inside_box", inside_o, inside_d)
    add("edges_corners", aim_o, aim_d)
    add("sides", side_o, side_d)
    add("spheres", sph_o, sph_d)
    return np.concatenate(o), np.concatenate(d), classes


def _unit(v):
    return v / np.linalg.norm(v)


def golden_rays(scene_id, sc, seed, n=3072):
    """rays of a golden scene that all hit something: random directions, axis-parallel ones, ones with a zero component of
    either sign, and rays from the camera into the scene.  Scenes 7 and 21 are a room open towards -z, where the camera
    stands: the rays start inside the bounds of its rectangles and never point towards -z.  Scene 23 is spheres and two
    lights over a ground sphere of radius 1000: the rays start above the ground and point downwards."""
    rng = np.random.default_rng(seed)
    cam = np.asarray(sc.camera["origin"], dtype=np.float64).reshape(3)
    k = n // 4
    if scene_id == 23:
        lo, hi = np.array([-6.0, 0.3, -6.0]), np.array([6.0, 8.0, 6.0])
        axes = np.array([[0.0, -1.0, 0.0], [-0.0, -1.0, 0.0], [0.0, -1.0, -0.0], [-0.0, -1.0, -0.0]])
        zeroed = (0, 2)
        aim_lo, aim_hi = np.array([-5.0, 0.0, -3.0]), np.array([5.0, 2.0, 3.0])
    else:
        nodes = sc.nodes
        ks = [nodes["f"][nodes["type"] == t][:, 4] for t in (A.NODE_YZ_RECT, A.NODE_XZ_RECT, A.NODE_XY_RECT)]
        lo, hi = np.array([q.min() for q in ks]), np.array([q.max() for q in ks])
        lo[2] = min(lo[2], 0.0)
        lo, hi = lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo)
        axes = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, -0.0, 0.0], [-0.0, -1.0, -0.0]])
        zeroed = (0, 1, 2)
        aim_lo, aim_hi = lo, hi

    def origins():
        return rng.uniform(lo, hi, (k, 3))

    o, d = [origins()], [rng.normal(size=(k, 3))]
    o.append(origins()), d.append(np.tile(axes, (k // len(axes) + 1, 1))[:k])
    dz = rng.normal(size=(k, 3))
    for q in range(k):
        dz[q, zeroed[q % len(zeroed)]] = 0.0 if (q // 3) % 2 else -0.0
    o.append(origins()), d.append(dz)
    o.append(np.tile(cam, (k, 1))), d.append(rng.uniform(aim_lo, aim_hi, (k, 3)) - cam)
    o, d = np.concatenate(o), np.concatenate(d)
    if scene_id == 23:
        # steep enough to meet the ground sphere (slope 0.3) or, every fourth ray, upwards into the light at y = 10 (2.5)
        flat = np.hypot(d[:, 0], d[:, 2])
        d[:, 1] = -(np.abs(d[:, 1]) + 0.3 * flat)
        up = np.arange(len(d)) % 4 == 3
        d[up, 1] = np.abs(d[up, 1]) + 2.2 * flat[up]
        # ... and some at the small light beside the spheres, from both of its sides
        m = 64
        src = np.stack([rng.uniform(1.0, 9.5, m), rng.uniform(2.0, 6.0, m), rng.uniform(0.0, 4.0, m)], axis=1)
        target = np.array([6.0, 4.0, 2.0]) + np.stack([np.zeros(m), rng.uniform(-0.2, 0.2, m), rng.uniform(-0.2, 0.2, m)], axis=1)
        o, d = np.concatenate([o, src]), np.concatenate([d, target - src])
    else:
        away = d[:, 2] < 0
        d[away, 2] = -d[away, 2]
    return o, d
