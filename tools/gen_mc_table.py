#!/usr/bin/env python
"""tools/gen_mc_table.py -- the marching-cubes case table of csrc/marching_cubes.hip (nr3d_lib_amd/csrc/mc_table.inc), constructed from
rules, not copied from anywhere.

Conventions
    corner c of a cell: offsets (dx, dy, dz) = (c & 1, (c >> 1) & 1, (c >> 2) & 1)
    case index = sum over corners of inside(c) << c            (inside: value < level)
    edge e = 4 a + u + 2 v: axis a, (u, v) = the offsets of its low end in the two OTHER dimensions, taken in rising order; the
        edge runs from p0 (p0[a] = 0) to p0 + e_a and is owned by the node at p0

Segments on the six faces.  Faces by dimension d = 0, 1, 2 and side s = 0, 1; their corners in the cyclic order (u, v) = (0, 0), (1, 0),
(1, 1), (0, 1) over the two other dimensions.  A face has 0, 2 or 4 sign-changing edges.  With 2: link the two.  With 4 (two diagonal
inside corners): cut every INSIDE corner off on its own, i.e. link the two face edges that meet at it.  The rule reads the face's four
signs only, so the two cells that share a face draw the same segments on it: that is what closes the mesh.

Loops and triangles.  Every crossed edge has degree 2.  Loops are traced from the lowest unvisited edge id, walking first to its
first-linked neighbour (links are made in the face order above; inside corners of a 4-face in the cyclic order).  A loop is oriented so
that its Newell normal (vertices at the edge midpoints) has a positive dot product with the sum over its edges of the unit vector from
the inside end to the outside end (non-zero in all 256 cases, asserted); re-orienting keeps the loop's first edge and reverses the
rest.  The loop is fan-triangulated from its first edge: (l0, l_i, l_i+1).  Triangle normals therefore point towards increasing value.

    python tools/gen_mc_table.py            # rewrite the .inc
    python tools/gen_mc_table.py --check    # exit 1 if the committed file differs

``tables()`` -> (TRI int8 [256, 16]: up to five triangles as edge ids, -1 padded; NTRI int32 [256]) for the test-side restatement.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "nr3d_lib_amd", "csrc", "mc_table.inc")
MAX_TRI = 5


def corner_offsets(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def corner_id(p):
    return p[0] | (p[1] << 1) | (p[2] << 2)


def edge_ends(e):
    """(p0, p1): the two corner offsets of edge e, low end first"""
    a, u, v = e >> 2, e & 1, (e >> 1) & 1
    p0 = [0, 0, 0]
    others = [d for d in range(3) if d != a]
    p0[others[0]], p0[others[1]] = u, v
    p1 = list(p0)
    p1[a] = 1
    return tuple(p0), tuple(p1)


def edge_between(p, q):
    """the id of the edge whose ends are the corner offsets p and q"""
    a = [d for d in range(3) if p[d] != q[d]]
    assert len(a) == 1
    a = a[0]
    others = [d for d in range(3) if d != a]
    return 4 * a + p[others[0]] + 2 * p[others[1]]


def face_corners(d, s):
    others = [k for k in range(3) if k != d]
    out = []
    for u, v in ((0, 0), (1, 0), (1, 1), (0, 1)):
        p = [0, 0, 0]
        p[d], p[others[0]], p[others[1]] = s, u, v
        out.append(tuple(p))
    return out


def case_links(case):
    """{edge: [neighbour, neighbour]} of the segments the six faces draw"""
    inside = [(case >> c) & 1 for c in range(8)]
    links = {}

    def link(a, b):
        links.setdefault(a, []).append(b)
        links.setdefault(b, []).append(a)

    for d in range(3):
        for s in range(2):
            q = face_corners(d, s)
            ins = [inside[corner_id(p)] for p in q]
            fe = [edge_between(q[m], q[(m + 1) % 4]) for m in range(4)]              # face edge m joins corners m and m + 1
            crossed = [m for m in range(4) if ins[m] != ins[(m + 1) % 4]]
            if len(crossed) == 2:
                link(fe[crossed[0]], fe[crossed[1]])
            elif len(crossed) == 4:
                for m in range(4):
                    if ins[m]:
                        link(fe[(m - 1) % 4], fe[m])
            else:
                assert not crossed
    return links


def case_loops(case):
    inside = [(case >> c) & 1 for c in range(8)]
    links = case_links(case)
    crossed = [e for e in range(12) if inside[corner_id(edge_ends(e)[0])] != inside[corner_id(edge_ends(e)[1])]]
    assert sorted(links) == crossed and all(len(v) == 2 for v in links.values()), case
    loops, seen = [], set()
    for e0 in crossed:
        if e0 in seen:
            continue
        loop, prev, cur = [e0], None, e0
        seen.add(e0)
        while True:
            a, b = links[cur]
            assert a != b, case                                                     # two edges share at most one face
            nxt = a if prev is None else (b if a == prev else a)
            if nxt == e0:
                break
            assert nxt not in seen, case
            loop.append(nxt)
            seen.add(nxt)
            prev, cur = cur, nxt
        assert len(loop) >= 3, case
        # orientation: Newell normal of the midpoints against the inside -> outside directions
        mid = []
        grad = [0, 0, 0]
        for e in loop:
            p0, p1 = edge_ends(e)
            mid.append([(p0[k] + p1[k]) / 2 for k in range(3)])
            sign = 1 if inside[corner_id(p0)] else -1                                # inside at the low end: outside lies towards +axis
            grad[e >> 2] += sign
        n = [0.0, 0.0, 0.0]
        for i in range(len(mid)):
            p, q = mid[i], mid[(i + 1) % len(mid)]
            n[0] += (p[1] - q[1]) * (p[2] + q[2])
            n[1] += (p[2] - q[2]) * (p[0] + q[0])
            n[2] += (p[0] - q[0]) * (p[1] + q[1])
        dot = sum(n[k] * grad[k] for k in range(3))
        assert dot != 0, case
        if dot < 0:
            loop = [loop[0]] + loop[:0:-1]
        loops.append(loop)
    return loops


def case_triangles(case):
    tris = []
    for loop in case_loops(case):
        for i in range(1, len(loop) - 1):
            tris.append((loop[0], loop[i], loop[i + 1]))
    assert len(tris) <= MAX_TRI, case
    return tris


def tables():
    import numpy as np
    tri = np.full((256, 16), -1, np.int8)
    ntri = np.zeros(256, np.int32)
    for case in range(256):
        t = case_triangles(case)
        ntri[case] = len(t)
        flat = [e for f in t for e in f]
        tri[case, :len(flat)] = flat
    return tri, ntri


def render():
    out = ["// GENERATED by tools/gen_mc_table.py -- do not edit.  Marching-cubes cases: corner c at offsets (c & 1, (c >> 1) & 1, (c >> 2) & 1),",
           "// case = sum of inside(c) << c, edge e = 4 axis + u + 2 v ((u, v): offsets of the low end in the two other dimensions); MC_TRI: up to",
           "// five triangles per case as edge ids, -1 padded, normals towards increasing value; MC_NTRI: their number.  See the generator.",
           f"#define NR3D_MC_MAX_TRI {MAX_TRI}",
           "static __device__ constexpr int8_t MC_TRI[256][16] = {"]
    ntri = []
    for case in range(256):
        t = case_triangles(case)
        ntri.append(len(t))
        flat = [e for f in t for e in f]
        flat += [-1] * (16 - len(flat))
        out.append("\t{ " + ", ".join("%2d" % e for e in flat) + " },   // %3d" % case)
    out.append("};")
    out.append("static __device__ constexpr uint8_t MC_NTRI[256] = {")
    for r in range(0, 256, 32):
        out.append("\t" + ", ".join(str(n) for n in ntri[r:r + 32]) + ",")
    out.append("};")
    return "\n".join(out) + "\n"


def main():
    text = render()
    if "--check" in sys.argv:
        ok = os.path.exists(OUT) and open(OUT).read() == text
        print(f"{OUT}: {'up to date' if ok else 'STALE'}")
        sys.exit(0 if ok else 1)
    if not os.path.exists(OUT) or open(OUT).read() != text:
        with open(OUT, "w") as f:
            f.write(text)
    print(f"{OUT}: 256 cases")


if __name__ == "__main__":
    main()
