"""An independent second opinion on the mesh loader (test infrastructure).

Written from the reference's GLSL alone -- vertex/loader.comp:32-152, include/structs.glsl:214-264 (MeshUniformStruct, the
accessor's component bits), include/vertex.glsl:194-207 (PICK: 16-bit indices, two to a word), include/mathlib.glsl:25,73-81
(mlength, mult4) and, for what the two matrices hold, VertexInstance.inl:55-56 (transform goes up transposed, transformInv as
glm::inverse leaves it, so `vec * mat` is T v for positions and inverse(T)^T n for normals) -- in plain Python on numpy float32
scalars, NOT from oracle/psm_oracle.c and not from bvh.hip / api.hip. Canonical rules it shares with the oracle by construction
(DESIGN.md 2.1): the `M.v` row (((m0 x + m1 y) + m2 z) + m3 w), the `dot` / `normalize` / `cross` row, `max(x, y) = x < y ? y : x`
(the "elsewhere" half of the min / max row); and the two rules the loader's own tests state: offsets are added as the GLSL's
uints (they wrap), a word outside the pool reads 0 (robust buffer access). INVERT_TX_Y is on, as the reference builds it.

load(mesh) -> (pos [n, 9], nrm [n, 9], mats [n], tex [n, 6]) over the dict that make_mesh_desc takes: what
oracle.load_mesh(mesh, with_tex=True) returns.
"""
import numpy as np

F = np.float32
U32 = 0xFFFFFFFF


def gl_max(x, y):
    return y if x < y else x


def mlength(c):  # mathlib.glsl:25
    return gl_max(c[0], gl_max(c[1], c[2]))


def dot(a, b):
    return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))


def cross(a, b):
    return (F(F(a[1] * b[2]) - F(b[1] * a[2])), F(F(a[2] * b[0]) - F(b[2] * a[0])), F(F(a[0] * b[1]) - F(b[0] * a[1])))


def normalize(a):
    inv = F(F(1.0) / F(np.sqrt(dot(a, a))))
    return (F(a[0] * inv), F(a[1] * inv), F(a[2] * inv))


def sub(a, b):
    return (F(a[0] - b[0]), F(a[1] - b[1]), F(a[2] - b[2]))


def load(mesh):
    verts = np.ascontiguousarray(mesh["vertices"], np.float32).reshape(-1)
    words = None if mesh.get("indices") is None else np.ascontiguousarray(mesh["indices"], np.uint32).reshape(-1)
    T = np.asarray(mesh["transform"], np.float32).reshape(4, 4)
    TI = np.asarray(mesh["transform_inv"], np.float32).reshape(4, 4)
    quads = mesh.get("primitive_type", 0) == 1
    nacc, tacc = mesh.get("normal_accessor", -1), mesh.get("texcoord_accessor", -1)

    def pool(i):
        return verts[i] if 0 <= i < verts.size else F(0.0)

    def read(accessor, idx):  # readByAccessor, :32-54
        offset4, cmps, view = mesh["accessors"][accessor]
        cmps &= 3                                                   # COMPONENTS = bits 0..1 (structs.glsl:250)
        voff, vstride = mesh["views"][view]
        stride4 = vstride if vstride > 0 else cmps + 1              # :36 (a signed compare: a negative stride is "none")
        at = (((idx * stride4 + voff) & U32) + offset4) & U32       # :39-42
        return [pool((at + k) & U32) if cmps >= k else F(0.0) for k in range(4)]

    def pick(i):  # :77
        if words is None:
            return i
        if mesh.get("index16", 0):
            w = int(words[i // 2]) if i // 2 < words.size else 0
            return (w >> (16 * (i & 1))) & 0xFFFF
        return int(words[i]) if i < words.size else 0

    with np.errstate(all="ignore"):
        pos, nrm, tex, mats = [], [], [], []
        trp = 4 if quads else 3                                     # :73
        for ctri in range(mesh["node_count"]):
            vertice, normal, texcoord = [], [], []
            for i in range(trp):
                v = pick((mesh.get("loading_offset", 0) + ctri * trp + i) & U32)
                p = read(mesh["vertex_accessor"], v)[:3]
                n = read(nacc, v)[:3] if nacc != -1 else [F(0.0)] * 3
                t = read(tacc, v)[:2] if tacc != -1 else [F(0.0)] * 2
                t[1] = F(F(1.0) - t[1])                              # :97-99
                # :101-103, v * mat: inverse(T)^T (n, 0) and T (p, 1)
                normal.append(tuple(F(F(F(F(TI[0][j] * n[0]) + F(TI[1][j] * n[1])) + F(TI[2][j] * n[2])) + F(TI[3][j] * F(0.0))) for j in range(3)))
                h = [F(F(F(F(T[j][0] * p[0]) + F(T[j][1] * p[1])) + F(T[j][2] * p[2])) + F(T[j][3] * F(1.0))) for j in range(4)]
                vertice.append((F(h[0] / h[3]), F(h[1] / h[3]), F(h[2] / h[3])))
                texcoord.append(tuple(t))
            face = normalize(normalize(cross(sub(vertice[1], vertice[0]), sub(vertice[2], vertice[0]))))   # :120, :128
            for order in ((0, 1, 2), (3, 0, 2))[: 2 if quads else 1]:                                      # :57, :136-151
                pp, nn, tt = [], [], []
                for mi in order:
                    n = normal[mi]
                    if mlength((abs(n[0]), abs(n[1]), abs(n[2]))) >= F(0.0001) and nacc != -1:       # :125
                        nn += list(normalize(n))
                    else:
                        nn += list(face)
                    pp += list(vertice[mi])
                    tt += list(texcoord[mi])
                pos.append(pp); nrm.append(nn); tex.append(tt); mats.append(mesh.get("material_id", 0))   # :65, :122
    n = len(mats)
    return (np.array(pos, np.float32).reshape(n, 9), np.array(nrm, np.float32).reshape(n, 9), np.array(mats, np.int32),
            np.array(tex, np.float32).reshape(n, 6))
