"""The split of a target range into chunks, pinned on the host: sh_nearest_points_chunks / _workspace and sh_nearest_surface_chunks /
_workspace against one transcription of the rule, over a grid that crosses every edge of it (no bodies, no queries, no targets,
one tile, one tile plus one, more workgroups than the chip holds, more chunks asked for than there are tiles)."""
import itertools

from semantichuman_amd import _lib

TILE = 256        # targets (triangles) per LDS tile, both searches
QT = 1024         # queries per workgroup, both searches
WG_SLOTS = 2048   # workgroups the chip holds at once

BS = (-1, 0, 1, 2, 16, 64, 65535)
NQS = (-1, 0, 1, 1023, 1024, 1025, 6890, 50000)
NTS = (-1, 0, 1, 255, 256, 257, 700, 6890, 13776, 20011, 55104)
CHUNKS = (0, 1, 2, 7, 79, 100000)


def cdiv(a, b):
    return -(-a // b)


def resolve_chunks(B, nq, nt, chunks):
    """The split actually run for a request of `chunks` (0 = automatic: as many chunks as fill the chip): whole tiles per chunk,
    no empty chunk."""
    tiles = cdiv(nt, TILE) if nt > 0 else 1
    c = chunks if chunks > 0 else cdiv(WG_SLOTS, cdiv(max(nq, 1), QT) * max(B, 1))
    c = max(1, min(c, tiles))
    return cdiv(tiles, cdiv(tiles, c))


def align16(v):
    return (v + 15) & ~15


def test_point_search_split_follows_the_rule():
    lib = _lib.load()
    for B, nq, nt in itertools.product(BS, NQS, NTS):
        # the point search does not split a search that has no body or no query
        want = 1 if B <= 0 or nq <= 0 else resolve_chunks(B, nq, nt, 0)
        assert lib.sh_nearest_points_chunks(B, nq, nt) == want, (B, nq, nt)
        for chunks in CHUNKS:
            c = resolve_chunks(B, nq, nt, chunks)
            want = 0 if B <= 0 or nq <= 0 or nt < 0 or c <= 1 else B * c * nq * 8
            assert lib.sh_nearest_points_workspace(B, nq, nt, chunks) == want, (B, nq, nt, chunks)


def test_surface_search_split_follows_the_rule():
    lib = _lib.load()
    for B, nq, nF in itertools.product(BS, NQS, NTS):
        assert lib.sh_nearest_surface_chunks(B, nq, nF) == resolve_chunks(B, nq, nF, 0), (B, nq, nF)
        for chunks in CHUNKS:
            c = resolve_chunks(B, nq, nF, chunks)
            want = 0 if B <= 0 or nq <= 0 or nF < 0 else align16(B * nF * 16) + align16(B * nF * 48) + B * c * nq * 8
            assert lib.sh_nearest_surface_workspace(B, nq, nF, chunks) == want, (B, nq, nF, chunks)
