"""The robot's visual meshes for the mesh renderer (rex_render_visual, csrc/rex_render_mesh.hip): file readers, per-file BVHs.

The reference draws the <visual> meshes of rex.urdf / rex_arm.urdf (RexGymEnv.render -> getCameraImage).  Which file rides on
which simulator body, where and in what colour is the generated table csrc/rex_visual_gen.h (tools/compile_model.py); the kernel
compiles it in and this module parses the same header, so there is one table.  The mesh files themselves are the reference's
data and are read at run time from the folder the caller names, as terrain.py reads heightfield files: `data_path` is what
rex_gym.util.pybullet_data.getDataPath() returns (the folder holding assets/urdf/).

One BVH per distinct file, shared by every instance that names it: a binary tree built by object-median splits along the
longest centroid axis, level by level with numpy (deterministic; ceil(log2(n / LEAF)) levels of inner nodes whatever the input,
so degenerate meshes cannot deepen it).  A node holds both children's boxes (the kernel visits the nearer child first):
16 dwords = lo0[3] hi0[3] lo1[3] hi1[3] c0 c1 0 0, where c >= 0 is an inner node and c < 0 a leaf, ~c = start << 3 | (count - 1).
Triangles are stored in leaf order as (v0, e1 = v1 - v0, e2 = v2 - v0) in metres: the mesh scale is applied when building,
so an instance's transform is the rigid pose of the table.
"""
import importlib.util
import os
import re
import struct
import time
import warnings

import numpy as np

LEAF = 4          # triangles per leaf at most
MAX_DEPTH = 32    # levels of inner nodes at most: the kernel's per-thread traversal stack (rex_render.h kMeshStack)
BOX_PAD = 1e-6    # [m] every box grows by this much (and by 2^-20 of its coordinates): the float32 triangles stay inside

_HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "rex_visual_gen.h")
KIND_BOX, KIND_CYL = 0, 1


# ---------------------------------------------------------------------------------------------------------------- the table
class VisualTable:
    """csrc/rex_visual_gen.h as arrays: entries 0..n_base-1 are mark 'base', all n_arm entries mark 'arm'."""

    def __init__(self, text):
        def define(name):
            return int(re.search(r"#define %s (\S+)" % name, text).group(1))

        def body(name):
            return re.search(r"%s\[[^=]*=\s*\{(.*?)\};" % name, text, re.S).group(1)

        def nums(name, cols=None):
            b = re.sub(r"/\*.*?\*/", "", body(name), flags=re.S)
            v = np.array([float(x) for x in re.findall(r"-?[0-9][0-9.eE+-]*", b)])
            return v if cols is None else v.reshape(-1, cols)

        self.n_base, self.n_arm = define("REX_VIS_N_BASE"), define("REX_VIS_N_ARM")
        self.body = nums("REX_VIS_BODY").astype(np.int64)
        self.pos, self.rot = nums("REX_VIS_POS", 3), nums("REX_VIS_ROT", 9).reshape(-1, 3, 3)
        self.rgb, self.scale = nums("REX_VIS_RGB", 3), nums("REX_VIS_SCALE")
        self.mesh = re.findall(r'"([^"]*)"', body("REX_VIS_MESH"))
        self.links = re.findall(r"/\* (\S+) \*/", body("REX_VIS_POS"))
        self.fb_kind = nums("REX_VIS_FB_KIND").astype(np.int64)
        self.fb_pos, self.fb_rot = nums("REX_VIS_FB_POS", 3), nums("REX_VIS_FB_ROT", 9).reshape(-1, 3, 3)
        self.fb_ext = nums("REX_VIS_FB_EXT", 3)
        for a in (self.body, self.pos, self.rot, self.rgb, self.scale, self.mesh, self.links, self.fb_kind, self.fb_pos,
                  self.fb_rot, self.fb_ext):
            assert len(a) == self.n_arm, "rex_visual_gen.h: malformed table"

    def count(self, mark):
        return self.n_arm if mark == "arm" else self.n_base


_TABLE = None


def visual_table():
    global _TABLE
    if _TABLE is None:
        with open(_HEADER) as f:
            _TABLE = VisualTable(f.read())
    return _TABLE


# -------------------------------------------------------------------------------------------------------------- the readers
def read_stl(path_or_bytes):
    """Binary or ASCII STL -> float64 [n, 3, 3].  Binary when the size is exactly 84 + 50 n (n = the count at byte 80): some
    binary files begin their 80-byte header with 'solid'.  A truncated or malformed file raises ValueError."""
    data = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else open(path_or_bytes, "rb").read()
    name = "STL data" if isinstance(path_or_bytes, (bytes, bytearray)) else path_or_bytes
    if len(data) >= 84:
        n = struct.unpack_from("<I", data, 80)[0]
        if len(data) == 84 + 50 * n:
            rec = np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")])
            return np.frombuffer(data, dtype=rec, count=n, offset=84)["v"].astype(np.float64)
    text = bytes(data).lstrip()
    if text[:5].lower() == b"solid":
        try:
            s = text.decode("ascii")
        except UnicodeDecodeError:
            s = None
        if s is not None and re.search(r"\bendsolid\b", s):
            facets = re.findall(r"\bfacet\b", s)
            ends = re.findall(r"\bendfacet\b", s)
            v = re.findall(r"\bvertex\s+(\S+)\s+(\S+)\s+(\S+)", s)
            if len(facets) == len(ends) and len(v) == 3 * len(ends):
                return np.array(v, dtype=np.float64).reshape(-1, 3, 3)
    raise ValueError(f"{name}: truncated or malformed STL ({len(data)} bytes)")


def read_obj(path_or_text):
    """Wavefront OBJ -> float64 [n, 3, 3]: 'v' lines and 'f' lines in the forms a, a/b, a//c and a/b/c, negative (relative)
    indices, polygons fan-triangulated.  Units as in the file."""
    text = path_or_text if "\n" in path_or_text else open(path_or_text).read()
    verts, faces = [], []
    for line in text.splitlines():
        t = line.split()
        if not t:
            continue
        if t[0] == "v":
            verts.append((float(t[1]), float(t[2]), float(t[3])))
        elif t[0] == "f":
            idx = []
            for tok in t[1:]:
                k = int(tok.split("/")[0])
                idx.append(k - 1 if k > 0 else len(verts) + k)
            if min(idx) < 0 or max(idx) >= len(verts):
                raise ValueError(f"OBJ face index out of range: {line!r}")
            for a in range(1, len(idx) - 1):
                faces.append((idx[0], idx[a], idx[a + 1]))
    v = np.array(verts, dtype=np.float64).reshape(-1, 3)
    return v[np.array(faces, dtype=np.int64).reshape(-1, 3)] if faces else np.zeros((0, 3, 3))


def read_mesh(path):
    return read_obj(path) if path.lower().endswith(".obj") else read_stl(path)


def tessellate(kind, ext, segments=48):
    """A collision primitive as triangles in its own frame: box (half extents ext) or cylinder about z (radius ext[0], half
    length ext[2]) with flat caps."""
    if kind == KIND_BOX:
        c = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64) * np.asarray(ext)
        quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
        return np.array([[c[q[0]], c[q[k]], c[q[k + 1]]] for q in quads for k in (1, 2)])
    r, h = float(ext[0]), float(ext[2])
    a = 2.0 * np.pi * np.arange(segments + 1) / segments
    ring = np.stack([r * np.cos(a), r * np.sin(a), np.zeros_like(a)], axis=1)
    lo, hi = ring + [0, 0, -h], ring + [0, 0, h]
    tri = []
    for k in range(segments):
        tri += [[lo[k], lo[k + 1], hi[k + 1]], [lo[k], hi[k + 1], hi[k]],
                [[0, 0, -h], lo[k + 1], lo[k]], [[0, 0, h], hi[k], hi[k + 1]]]
    return np.array(tri, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------ the BVH
class Bvh:
    """nodes: float32 [m, 16] (the int fields through .view(np.int32)); tris: float32 [n, 9] (v0, e1, e2) in leaf order;
    order: the source triangle of every stored one; depth: levels of inner nodes; lo / hi: the root box (float32 [3])."""

    def __init__(self, nodes, tris, order, depth, lo, hi):
        self.nodes, self.tris, self.order, self.depth, self.lo, self.hi = nodes, tris, order, depth, lo, hi


def _leaf(start, count):
    return ~((start << 3) | (count - 1))


def _round_out(lo, hi):
    # grow by BOX_PAD plus 2^-20 of the magnitude (v0 + e1 in float32 lands within a few ulp of v1), then round outwards
    pad = BOX_PAD + 2.0 ** -20 * np.maximum(np.abs(lo), np.abs(hi))
    lo, hi = lo - pad, hi + pad
    lo32, hi32 = lo.astype(np.float32), hi.astype(np.float32)
    lo32 = np.where(lo32 > lo, np.nextafter(lo32, np.float32(-np.inf)), lo32)
    hi32 = np.where(hi32 < hi, np.nextafter(hi32, np.float32(np.inf)), hi32)
    return lo32, hi32


def build_bvh(tris, leaf=LEAF, max_depth=MAX_DEPTH):
    """Triangles float64 [n, 3, 3] -> Bvh.  Deterministic (stable sorts only).  Raises ValueError if the tree would need
    more than max_depth levels of inner nodes."""
    if not 1 <= leaf <= 8:
        raise ValueError("leaf size must be 1..8 (3 bits of the leaf code)")
    tris = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    n = len(tris)
    if n == 0:
        return Bvh(np.zeros((0, 16), np.float32), np.zeros((0, 9), np.float32), np.zeros(0, np.int64), 0,
                   np.zeros(3, np.float32), np.zeros(3, np.float32))
    if n >= 1 << 28:
        raise ValueError("too many triangles for the leaf code (2^28)")
    tlo, thi = tris.min(axis=1), tris.max(axis=1)
    cen = 0.5 * (tlo + thi)
    perm = np.arange(n)
    bounds = np.array([0, n])           # the current partition of the (permuted) triangles
    levels = []                          # per level: starts, mids, ends of its inner nodes
    while True:
        starts, ends = bounds[:-1], bounds[1:]
        size = ends - starts
        active = size > leaf if levels else np.array([True])
        if not active.any():
            break
        if len(levels) >= max_depth:
            raise ValueError(f"BVH deeper than {max_depth} levels")
        seg = np.repeat(np.arange(len(starts)), size)
        cp = cen[perm]
        ext = np.maximum.reduceat(cp, starts) - np.minimum.reduceat(cp, starts)
        axis = np.argmax(ext, axis=1)
        key = np.where(active[seg], cp[np.arange(n), axis[seg]], 0.0)
        perm = perm[np.lexsort((key, seg))]
        mids = starts[active] + (size[active] + 1) // 2
        if not levels and n <= leaf:
            mids = np.array([n])        # a single leaf: the root's two children are the same range
        bounds = np.unique(np.concatenate([bounds, mids]))
        levels.append((starts[active], mids, ends[active], bounds))
    first = np.cumsum([0] + [len(l[0]) for l in levels])
    m = int(first[-1])
    nodes = np.zeros((m, 16), np.float32)
    ni = nodes.view(np.int32)
    lo_p, hi_p = tlo[perm], thi[perm]
    for d, (s, mid, e, bnd) in enumerate(levels):
        cs = [(s, e), (s, e)] if n <= leaf else [(s, mid), (mid, e)]
        nxt = levels[d + 1] if d + 1 < len(levels) else (np.zeros(0, np.int64),)
        seg_lo, seg_hi = np.minimum.reduceat(lo_p, bnd[:-1]), np.maximum.reduceat(hi_p, bnd[:-1])   # the children are segments of bnd
        for c, (a, b) in enumerate(cs):
            k = np.searchsorted(bnd, a)
            assert (bnd[k + 1] == b).all()
            lo32, hi32 = _round_out(seg_lo[k], seg_hi[k])
            idx = np.arange(first[d], first[d + 1])
            nodes[idx, 6 * c:6 * c + 3], nodes[idx, 6 * c + 3:6 * c + 6] = lo32, hi32
            inner = (b - a) > leaf
            rank = np.searchsorted(nxt[0], a)       # the next level's inner nodes, in order of their start
            code = np.where(inner, first[d + 1] + rank, _leaf(a, np.maximum(b - a, 1)))
            ni[idx, 12 + c] = code.astype(np.int32)
    v = tris[perm]
    out = np.concatenate([v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]], axis=1).astype(np.float32)
    rlo, rhi = _round_out(tlo.min(axis=0, keepdims=True), thi.max(axis=0, keepdims=True))
    return Bvh(nodes, np.ascontiguousarray(out), perm, len(levels), rlo[0], rhi[0])


# --------------------------------------------------------------------------------------------------------------- the loader
_CACHE = {}   # (path, size, mtime_ns, scale) -> Bvh: parsed and built once per process


def default_data_path():
    """rex_gym.util.pybullet_data.getDataPath() of an installed reference, found without importing it (or None)."""
    spec = importlib.util.find_spec("rex_gym")
    if spec is None or not spec.submodule_search_locations:
        return None
    return os.path.join(list(spec.submodule_search_locations)[0], "util", "pybullet_data")


def mesh_bvh(path, scale):
    st = os.stat(path)
    key = (os.path.abspath(path), st.st_size, st.st_mtime_ns, float(scale))
    if key not in _CACHE:
        _CACHE[key] = build_bvh(read_mesh(path) * float(scale))
    return _CACHE[key]


def fallback_bvh(table, k):
    """Entry k's collision primitive, tessellated and placed in the entry's mesh frame (empty if the link has none)."""
    key = ("fallback", k)
    if key not in _CACHE:
        if table.fb_kind[k] < 0:
            tri = np.zeros((0, 3, 3))
        else:   # primitive frame -> body frame -> mesh frame: p_mesh = R_vis^T (p_body - t_vis)
            body = tessellate(table.fb_kind[k], table.fb_ext[k]) @ table.fb_rot[k].T + table.fb_pos[k]
            tri = (body - table.pos[k]) @ table.rot[k]
        _CACHE[key] = build_bvh(tri)
    return _CACHE[key]


class VisualMeshes:
    """What rex_render_set_visuals takes, for one mark: nodes float32 [m, 16], tris float32 [t, 9], and per instance (table
    entry) its root node (-1: an empty mesh) and its mesh-frame root box lo / hi float32 [k, 3].  .missing lists the files
    that were not found (drawn as their link's collision primitive); .seconds the time the load took on this host."""

    def __init__(self, mark, data_path, entries, missing, seconds):
        self.mark, self.data_path, self.missing, self.seconds = mark, data_path, missing, seconds
        nodes, tris, root, lo, hi, seen = [], [], [], [], [], {}
        n_nodes = n_tris = 0
        self.depth = 0
        for key, b in entries:
            if key not in seen:
                seen[key] = (n_nodes, n_tris)
                nd = b.nodes.copy()
                ni = nd.view(np.int32)
                c = ni[:, 12:14]
                start, count = (~c) >> 3, (~c) & 7
                ni[:, 12:14] = np.where(c >= 0, c + n_nodes, ~(((start + n_tris) << 3) | count))
                nodes.append(nd)
                tris.append(b.tris)
                n_nodes += len(b.nodes)
                n_tris += len(b.tris)
                self.depth = max(self.depth, b.depth)
            root.append(seen[key][0] if len(b.nodes) else -1)
            lo.append(b.lo)
            hi.append(b.hi)
        self.nodes = np.ascontiguousarray(np.concatenate(nodes) if nodes else np.zeros((0, 16), np.float32))
        self.tris = np.ascontiguousarray(np.concatenate(tris) if tris else np.zeros((0, 9), np.float32))
        self.root = np.array(root, dtype=np.int32)
        self.lo, self.hi = np.array(lo, dtype=np.float32), np.array(hi, dtype=np.float32)
        self.distinct = len(seen)


def load(data_path=None, mark="base"):
    """Read and build the visual meshes of one mark ('base': rex.urdf's 23 visuals; 'arm': rex_arm.urdf's 29).  data_path =
    rex_gym.util.pybullet_data.getDataPath() (default: that of an installed rex_gym).  A missing file is drawn as its
    link's collision primitive, listed in .missing and reported by one warning."""
    if data_path is None:
        data_path = default_data_path()
        if data_path is None:
            raise ValueError("load_visual_meshes: pass data_path=<the folder holding assets/urdf/, i.e. "
                             "rex_gym.util.pybullet_data.getDataPath()>: rex_gym is not installed")
    urdf_dir = os.path.join(data_path, "assets", "urdf")
    if not os.path.isdir(urdf_dir):
        raise ValueError(f"load_visual_meshes: data_path {data_path!r} holds no assets/urdf/ folder")
    t0 = time.perf_counter()
    table = visual_table()
    entries, missing = [], []
    for k in range(table.count(mark)):
        path = os.path.join(urdf_dir, table.mesh[k])
        if os.path.exists(path):
            entries.append((table.mesh[k], mesh_bvh(path, table.scale[k])))
        else:
            if table.mesh[k] not in missing:
                missing.append(table.mesh[k])
            entries.append((("fallback", k), fallback_bvh(table, k)))
    if missing:
        warnings.warn(f"visual meshes not found under {urdf_dir}: {', '.join(missing)}; drawn as their links' collision primitives",
                      stacklevel=2)
    return VisualMeshes(mark, data_path, entries, missing, time.perf_counter() - t0)
