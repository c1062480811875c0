"""Plain-Python oracle of sfm_build_tracks (csrc/sfm_track_build.hip): a union-find by rank with full path
compression over the matches, then the contract's rules written out directly.  It shares no structure with the device
algorithm (no hooking by id, no radix sort)."""
import numpy as np

OK, UNMATCHED, CONFLICT, BAD_INDEX = 0, 1, 2, 3


class UnionFind:
    def __init__(self, n: int):
        self.parent = list(range(n))
        self.rank = [0] * n

    def find(self, v: int) -> int:
        root = v
        while self.parent[root] != root:
            root = self.parent[root]
        while self.parent[v] != root:   # full path compression
            self.parent[v], v = root, self.parent[v]
        return root

    def union(self, a: int, b: int) -> None:
        ra, rb = self.find(a), self.find(b)
        if ra == rb:
            return
        if self.rank[ra] < self.rank[rb]:
            ra, rb = rb, ra
        self.parent[rb] = ra
        if self.rank[ra] == self.rank[rb]:
            self.rank[ra] += 1


def global_edges(image_offset, pairs, match_offset, match_index):
    """(E, 2) global ids of the matches, or None when an input is out of range."""
    off = np.asarray(image_offset, dtype=np.int64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    mo = np.asarray(match_offset, dtype=np.int64)
    mi = np.asarray(match_index, dtype=np.int64).reshape(-1, 2)
    I, Q, E = len(off) - 1, len(pairs), len(mi)
    if off[0] != 0 or np.any(np.diff(off) < 0) or mo[0] != 0 or mo[-1] != E or np.any(np.diff(mo) < 0) or len(mo) != Q + 1:
        return None
    if Q and (pairs.min() < 0 or pairs.max() >= I or np.any(pairs[:, 0] == pairs[:, 1])):
        return None
    owner = np.repeat(np.arange(Q), np.diff(mo))
    if E == 0:
        return np.zeros((0, 2), dtype=np.int64)
    ia, ib = pairs[owner, 0], pairs[owner, 1]
    n = np.diff(off)
    if mi.min() < 0 or np.any(mi[:, 0] >= n[ia]) or np.any(mi[:, 1] >= n[ib]):
        return None
    return np.column_stack([off[ia] + mi[:, 0], off[ib] + mi[:, 1]])


def build_tracks(image_offset, pairs, match_offset, match_index):
    """dict(component, status, track, camera_index, point_index, feature_index (each [F], the last three -1 past M),
    info (status, components, tracks, observations, conflicts, unmatched))."""
    off = np.asarray(image_offset, dtype=np.int64)
    F = int(off[-1])
    minus = np.full(F, -1, dtype=np.int64)
    edges = global_edges(image_offset, pairs, match_offset, match_index)
    if edges is None:
        return dict(component=minus.copy(), status=np.full(F, BAD_INDEX, dtype=np.uint8), track=minus.copy(),
                    camera_index=minus.copy(), point_index=minus.copy(), feature_index=minus.copy(), info=(1, 0, 0, 0, 0, 0))
    uf = UnionFind(F)
    for a, b in edges.tolist():
        uf.union(a, b)
    root = np.array([uf.find(g) for g in range(F)], dtype=np.int64)
    smallest = np.full(F, F, dtype=np.int64)
    np.minimum.at(smallest, root, np.arange(F))
    component = smallest[root] if F else minus.copy()
    image = np.repeat(np.arange(len(off) - 1), np.diff(off))
    size = np.bincount(component, minlength=F) if F else np.zeros(0, dtype=np.int64)
    # a component holds two features of one image: some (component, image) occurs twice
    key = component * max(len(off) - 1, 1) + image
    u, c = np.unique(key, return_counts=True)
    bad_comp = np.zeros(F, dtype=bool)
    bad_comp[u[c > 1] // max(len(off) - 1, 1)] = True
    status = np.where(size[component] == 1, UNMATCHED, np.where(bad_comp[component], CONFLICT, OK)).astype(np.uint8)
    ok_components = np.unique(component[status == OK])   # increasing component id = track id order
    track_of_component = np.full(F, -1, dtype=np.int64)
    track_of_component[ok_components] = np.arange(len(ok_components))
    track = np.where(status == OK, track_of_component[component], -1)
    members = np.nonzero(status == OK)[0]
    order = np.lexsort((members, track[members]))   # by track, then by global id
    fid = members[order]
    M = len(fid)
    cam, pt, fi = minus.copy(), minus.copy(), minus.copy()
    cam[:M], pt[:M], fi[:M] = image[fid], track[fid], fid
    roots = np.unique(component)
    info = (0, int(np.count_nonzero(size[roots] >= 2)), len(ok_components), M, int(np.count_nonzero(bad_comp[roots])),
            int(np.count_nonzero(status == UNMATCHED)))
    return dict(component=component, status=status, track=track, camera_index=cam, point_index=pt, feature_index=fi,
                info=info)


def from_lists(counts, pairs, matches):
    """(image_offset, pairs, match_offset, match_index) from per-image feature counts and per-pair (n, 2) match arrays."""
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    lens = [len(m) for m in matches]
    mo = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    mi = np.concatenate([np.asarray(m, dtype=np.int64).reshape(-1, 2) for m in matches]) if matches else np.zeros((0, 2))
    return off, pairs, mo, mi.astype(np.int64).reshape(-1, 2)
