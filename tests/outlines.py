"""Other racket outlines for the parity tests (the product's comes from racket.stl: 38 edges)."""
import numpy as np


def with_vertices(p, verts, half_thick=None):
    """`p` with the outline given by explicit CCW (y, z) vertices about the COM (edge i runs from vertex i to vertex i + 1; collinear
    vertices are allowed: the ball narrowphase only needs every edge's interior on its left), optionally another half thickness, and
    the derived fields set as params.default_params sets them"""
    from tennisbot_rl_amd.params import hull_edge_table
    rec = hull_edge_table(np.asarray(verts, np.float64), (0.0, 0.0), 1.0)
    q = p.copy()
    if half_thick is not None:
        q.racket_half_thick = float(half_thick)
    q.n_hull = len(rec)
    e = np.ctypeslib.as_array(q.hull_edges)
    e[:] = 0.0
    e[:len(rec)] = rec
    vmax = float(np.sqrt((rec[:, :2].astype(np.float64) ** 2).sum(1).max() + float(q.racket_half_thick) ** 2))
    q.hull_bound_radius = vmax * 1.0001
    q.racket_ground_threshold = 0.02 * vmax
    return q


def rectangle(p, half_y=0.125, half_z=0.25, half_thick=1.0 / 64.0, cuts_y=(), cuts_z=()):
    """a rectangular outline whose edge 0 is the +y side (normal +y), then +z, -y, -z. cuts_z / cuts_y: piece lengths that cut the
    +-y sides (along z) / the +-z sides (along y) into collinear edges; with dyadic lengths every vertex, edge and reciprocal length
    is exact in float32. Empty cuts: the plain 4-edge rectangle."""
    cz, cy = list(cuts_z) or [2.0 * half_z], list(cuts_y) or [2.0 * half_y]
    assert abs(sum(cz) - 2.0 * half_z) == 0.0 and abs(sum(cy) - 2.0 * half_y) == 0.0
    v, z, y = [], -half_z, half_y
    for c in cz:          # the +y side, upwards
        v.append((half_y, z)); z += c
    for c in cy:          # the +z side, towards -y
        v.append((y, half_z)); y -= c
    for c in cz:          # the -y side, downwards
        v.append((-half_y, z)); z -= c
    for c in cy:          # the -z side, towards +y
        v.append((y, -half_z)); y += c
    return with_vertices(p, v, half_thick)


def with_outline(p, n_edges, radius_y=0.13, radius_z=0.33):
    """`p` with another racket outline: a convex n-gon (an ellipse sampled at uneven angles), CCW in (y, z) about the COM, with the
    fields params.default_params derives from the outline set the same way"""
    from tennisbot_rl_amd.params import hull_edge_table
    rng = np.random.default_rng(100 + n_edges)
    ang = np.sort((np.arange(n_edges) + rng.uniform(-0.3, 0.3, n_edges)) * (2.0 * np.pi / n_edges))
    verts = np.stack([radius_y * np.cos(ang), radius_z * np.sin(ang)], 1)
    rec = hull_edge_table(verts, (0.0, 0.0), 1.0)
    q = p.copy()
    q.n_hull = n_edges
    e = np.ctypeslib.as_array(q.hull_edges)
    e[:] = 0.0
    e[:n_edges] = rec
    vmax = float(np.sqrt((rec[:, :2].astype(np.float64) ** 2).sum(1).max() + float(q.racket_half_thick) ** 2))
    q.hull_bound_radius = vmax * 1.0001
    q.racket_ground_threshold = 0.02 * vmax
    return q
