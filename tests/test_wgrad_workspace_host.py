"""sh_spiral_conv_bwd_wgt_workspace pinned on the host: the bytes of partial slabs the fp32 spiral-conv weight gradient writes, as
literal counts, one shape per regime of the kernel choice (choose_wgrad in csrc/spiral_conv.hip).  Stack arenas, the thin-layer
kernel and the deferred reduction count slabs by this plan: a count that moves resizes every arena and changes the order of the
slab sums, and with it the bits of every weight gradient."""
from semantichuman_amd import _lib

# (B, R, S, Cin, Cout) -> bytes = slabs x (Cout x S x Cin + Cout) x 4
WORKSPACE = {
    (2, 64, 4, 5, 7): 2352,                # staged form (Cin neither a multiple of 4 nor 3): 4 slabs
    (2, 64, 5, 14, 32): 36352,             # ... with 128-wide column groups: 4 slabs
    (48, 431, 9, 32, 32): 6880512,         # streaming form, 3 batch slices: the plain strided walk, 186 slabs
    (16, 40, 9, 32, 32): 1479680,          # one vertex range per XCD, 1 batch slice: 8 x 5 slabs
    (32, 40, 9, 32, 32): 2959360,          # ... 2 slices: 8 x 10
    (64, 40, 9, 32, 32): 5918720,          # ... 4 slices: 8 x 20
    (128, 40, 9, 32, 32): 7398400,         # ... 8 slices: 8 x 25, one round of the item target
    (64, 3446, 9, 32, 32): 7398400,        # a headline layer: 200 slabs
    (64, 6890, 9, 16, 3): 890880,          # the 16 -> 3 layer: 1536 items, 512 slabs
    (64, 3446, 9, 64, 272): 70310912,      # the slab budget binds (it can only above 128 output channels): 112 slabs
    (64, 27554, 18, 32, 32): 75628544,     # the table cap forces whole extra rounds: 1024 slabs
    (64, 6890, 9, 3, 16): 1835008,         # 3-channel input, columns in padded quads: 1024 slabs
    (64, 431, 9, 32, 160): 36992000,       # more than 128 output channels, two launches on the same 200 slabs
    (0, 431, 9, 32, 32): 0,                # a non-positive size
    (64, 431, 9, 32, -1): 0,
    (64, 431, 0, 32, 32): 0,
}


def test_wgrad_workspace_bytes():
    lib = _lib.load()
    got = {shape: int(lib.sh_spiral_conv_bwd_wgt_workspace(*shape)) for shape in WORKSPACE}
    assert got == WORKSPACE
