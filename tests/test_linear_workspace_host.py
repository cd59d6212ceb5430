"""sh_linear_workspace pinned on the host: the bytes a split reduction of any of the three latent-FC passes may need, as literal
counts, one shape per regime of the kernel choice in csrc/linear.hip.  Stack arenas and the benchmark are sized by this function;
the counts were taken from the library before the choice moved into one place and must not move with it."""
from semantichuman_amd import _lib

# (M, N, K) -> bytes = splits x rows x cols x 4 of the largest slab among forward [M][N], backward-data [M][K], weight gradient [N][K]
WORKSPACE = {
    (64, 256, 55296): 16187392,      # encoder latent layer, batch 64: forward streams K in 247 ranges of 224
    (64, 55296, 256): 16187392,      # decoder latent layer, batch 64: backward-data streams N the same way
    (1024, 55296, 256): 16777216,    # the decode batch: the generic kernel's backward-data, 16 chunks of 3456
    (5, 64, 1040): 21760,            # streaming forward, 16-granular ranges: 17 splits
    (5, 256, 1056): 87040,           # streaming forward, 32-granular ranges (LDS-DMA and bf16x3 forms): 17 splits
    (33, 1056, 256): 574464,         # streaming backward-data: 17 splits
    (4, 8, 2048): 1024,              # generic kernel, forward: 8 splits
    (3, 5, 2050): 540,               # ... with a last chunk of 2: 9 splits
    (2048, 64, 64): 131072,          # generic kernel, weight gradient: 8 splits
    (17, 64, 64): 0,                 # nothing is split
    (65, 256, 416): 0,               # the chunked forward is never split
    (0, 64, 64): 0,                  # a non-positive dimension
    (64, -1, 64): 0,
    (64, 64, 0): 0,
}


def test_linear_workspace_bytes():
    lib = _lib.load()
    got = {shape: int(lib.sh_linear_workspace(*shape)) for shape in WORKSPACE}
    assert got == WORKSPACE
