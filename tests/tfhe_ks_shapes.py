"""Shapes of the LWE key switch (csrc/pfhe_bootstrap.hip, tfhe_keyswitch_kernel) at which its loops take their other paths,
shared by tests/test_tfhe_bootstrap_shapes_cpu.py (which proves that the table holds them) and
tests/test_gpu_tfhe_bootstrap_edges.py (which runs them).  Nothing here imports the library.

The kernel walks the mask words in groups of ki (ki * ell <= 64, at most 8 mask words per group).  A group of
g mask words has g * ell key rows; the kernel takes them four at a time and finishes the rest one by one.

The private key switch (csrc/pfhe_cbs.hip, tfhe_pfks_kernel) runs the same tile over in_dim + 1 words, the body included:
tests/tfhe_cbs_model.py takes the constants and both functions from here and keeps its own table of shapes.
"""

KS_MAX_ROWS = 64        # key rows of one group, the LDS bound
KS_MAX_WORDS = 8        # mask words of one group: 256 threads / 32 ciphertexts of a tile
KS_UNROLL = 4           # key rows in flight
KS_TILE_BATCH = 32      # ciphertexts of one workgroup
KS_TILE_COLS = 128      # output columns of one workgroup, two per lane 64 apart

# bits, in_dim, out_dim, log_basis, ell, batch                      ki   rows per group
KS_EDGE_SHAPES = [
    (32, 13, 127, 4, 3, 33),                                      #  8   24, 15
    (32, 3, 128, 5, 5, 31),                                       #  8   15
    (32, 1, 1, 4, 3, 1),                                          #  8   3: the unrolled loop never runs
    (32, 17, 4, 6, 5, 32),                                        #  8   40, 40, 5
    (32, 9, 5, 5, 6, 4),                                          #  8   48, 6
    (32, 9, 1, 2, 11, 64),                                        #  5   55, 44
    (64, 19, 3, 9, 7, 2),                                         #  8   56, 56, 21
    (64, 11, 2, 5, 9, 32),                                        #  7   63, 36
    (64, 13, 9, 3, 10, 6),                                        #  6   60, 60, 10
    (64, 6, 2, 4, 15, 2),                                         #  4   60, 30
    (64, 7, 255, 3, 17, 5),                                       #  3   51, 51, 17
    (64, 10, 7, 2, 21, 3),                                        #  3   63, 63, 63, 21
    (64, 5, 256, 1, 33, 9),                                       #  1   33 each
]


def group_words(ell: int) -> int:
    """ki: mask words per group"""
    return max(1, min(KS_MAX_ROWS // ell, KS_MAX_WORDS))


def group_rows(in_dim: int, ell: int):
    """key rows of every group, in the order the kernel walks them"""
    ki = group_words(ell)
    return [min(ki, in_dim - i0) * ell for i0 in range(0, in_dim, ki)]
