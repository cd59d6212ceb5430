"""What choose_p3 (csrc/p3_conv.hip) makes of a shape, pinned on the host through the predicates that read it: one shape
per regime of the choice - 16 gathered channels, 1 / 2 / 4 / 8 channel tiles per workgroup, the streamed weight with and without
K padding, every refused row of tests/test_p3_shapes.py's GRID - and the near misses next to them.  Stack arenas are planned from
these answers (stack.py, stack_exec.hip): a value that moves resizes a fragment buffer or sends a layer to another kernel.  The
literals were recorded from the library before the choice moved into one routine."""
from semantichuman_amd import _lib

# (B, S, Cg, Nout) -> (sh_spiral_conv_p3_ok, _p3_kind, _p3_rag_ok at lists of 8 / 64 / 65, _p3_grp_ok at 8 / 64 / 65, _p3_grp_members,
#                      sh_conv_wfrag3_bytes(S, Cg, Nout), sh_p3_bytes(7, B, Cg), sh_p3_bytes(7, B, Nout))
CHOICE = {
    (64, 9, 16, 32): (1, 1, (0, 0, 0), (1, 1, 0), 4, 30720, 43008, 86016),              # 16 gathered channels, two tiles
    (16, 12, 32, 12): (1, 1, (1, 1, 0), (1, 1, 0), 4, 36864, 21504, 0),                 # one channel tile per workgroup
    (64, 3, 128, 32): (1, 1, (1, 1, 0), (1, 1, 0), 4, 73728, 344064, 86016),            # two
    (64, 4, 96, 64): (1, 1, (1, 1, 0), (1, 1, 0), 2, 147456, 258048, 172032),           # four: groups of two members
    (80, 3, 32, 128): (1, 1, (0, 0, 0), (0, 0, 0), 0, 73728, 107520, 430080),           # eight: no list kernel
    (64, 12, 64, 64): (1, 2, (0, 0, 0), (0, 0, 0), 0, 294912, 172032, 172032),          # streamed, K in whole chunks
    (48, 25, 32, 64): (1, 2, (0, 0, 0), (0, 0, 0), 0, 344064, 64512, 129024),           # streamed, K padded from 25 to 28 k-steps
    (16, 9, 256, 32): (1, 2, (0, 0, 0), (0, 0, 0), 0, 442368, 172032, 21504),           # streamed, 32 output channels (two tiles)
    # refused (GRID's rej rows): the fragment buffer still has a size
    (40, 8, 32, 32): (0, 0, (0, 0, 0), (0, 0, 0), 0, 49152, 0, 0),                      # rej_b40
    (64, 8, 32, 30): (0, 0, (0, 0, 0), (0, 0, 0), 0, 49152, 86016, 0),                  # rej_n30
    (64, 8, 48, 32): (0, 0, (0, 0, 0), (0, 0, 0), 0, 73728, 0, 86016),                  # rej_c48
    (64, 65, 16, 16): (0, 0, (0, 0, 0), (0, 0, 0), 0, 101376, 43008, 43008),            # rej_s65
    (64, 9, 16, 64): (0, 0, (0, 0, 0), (0, 0, 0), 0, 61440, 43008, 172032),             # rej_c16_n64: four tiles at 16 channels are not built
    (48, 9, 96, 96): (0, 0, (0, 0, 0), (0, 0, 0), 0, 663552, 193536, 193536),           # rej_c96_n96: neither resident nor streamed
    (48, 3, 96, 96): (0, 0, (0, 0, 0), (0, 0, 0), 0, 221184, 193536, 193536),           # w_r5
    # near misses
    (64, 9, 16, 48): (0, 0, (0, 0, 0), (0, 0, 0), 0, 61440, 43008, 0),                  # 16 gathered channels, 48 output channels
    (64, 3, 32, 48): (1, 1, (1, 1, 0), (1, 1, 0), 2, 36864, 86016, 0),                  # 3 tiles of output channels run as 4
    (64, 3, 32, 80): (1, 1, (0, 0, 0), (0, 0, 0), 0, 73728, 86016, 0),                  # 5 as 8
    (64, 3, 32, 96): (1, 1, (0, 0, 0), (0, 0, 0), 0, 73728, 86016, 258048),             # 6 as 8
    (32, 64, 16, 12): (1, 1, (0, 0, 0), (1, 1, 0), 4, 98304, 21504, 0),                 # the longest spiral, resident
    (32, 65, 16, 12): (0, 0, (0, 0, 0), (0, 0, 0), 0, 101376, 21504, 0),                # one past it
    (32, 64, 32, 64): (1, 2, (0, 0, 0), (0, 0, 0), 0, 786432, 43008, 86016),            # the longest spiral, streamed
    (32, 65, 32, 64): (0, 0, (0, 0, 0), (0, 0, 0), 0, 835584, 43008, 86016),            # one past it
}

# (B, n_groups) -> sh_spiral_conv_p3_grp_pays: 12 items per CU, at the 256 CUs of an MI355X (and of a host without a device)
PAYS = {(64, 767): 0, (64, 768): 1, (16, 3071): 0, (16, 3072): 1, (8, 100000): 0, (40, 1535): 0, (40, 1536): 1, (1024, 47): 0,
        (1024, 48): 1, (0, 5000): 0}


def test_p3_choice_through_the_predicates():
    lib = _lib.load()
    got = {}
    for B, S, Cg, Nout in CHOICE:
        got[(B, S, Cg, Nout)] = (lib.sh_spiral_conv_p3_ok(B, S, Cg, Nout), lib.sh_spiral_conv_p3_kind(B, S, Cg, Nout),
                                 tuple(lib.sh_spiral_conv_p3_rag_ok(B, S, Cg, Nout, L) for L in (8, 64, 65)),
                                 tuple(lib.sh_spiral_conv_p3_grp_ok(B, S, Cg, Nout, L) for L in (8, 64, 65)),
                                 lib.sh_spiral_conv_p3_grp_members(B, S, Cg, Nout), int(lib.sh_conv_wfrag3_bytes(S, Cg, Nout)),
                                 int(lib.sh_p3_bytes(7, B, Cg)), int(lib.sh_p3_bytes(7, B, Nout)))
    assert got == CHOICE


def test_p3_grouping_pays_at_256_cus():
    lib = _lib.load()
    assert {k: lib.sh_spiral_conv_p3_grp_pays(*k) for k in PAYS} == PAYS
