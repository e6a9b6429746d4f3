"""The (V, K) block matrix of test_gpu_partitions.py as a plain table (no test
module is imported here, so the CPU descriptor test in test_capi.py can read it)."""

D3 = "distance d=3"  # K = 4, from graph.get_normalized_adjacency_matrices(1, 3)

CASES = {
    # id: (C_in, C_out, stride, V, A key, K, N, T)
    "a": (64, 64, 1, 18, "s1_d1", 2, 2, 12),
    "b": (64, 64, 1, 18, "s1_d1", 2, 2, 21),
    "c": (64, 128, 2, 18, "s2_d1", 3, 2, 13),
    "d": (64, 64, 1, 18, "s1_d2", 3, 2, 12),
    "e": (3, 64, 1, 18, "s2_d1", 3, 3, 15),
    "f": (64, 64, 1, 25, "s1_d1", 2, 2, 12),
    "g": (32, 64, 2, 25, "s3_d1", 2, 3, 11),
    "h": (64, 64, 1, 25, "s1_d1", 2, 2, 21),
    "i": (3, 64, 1, 25, "s1_d1", 2, 3, 15),
    "j": (64, 64, 1, 25, "s0_d2", 1, 2, 12),
    "k": (64, 64, 1, 50, "s1_d1", 2, 2, 8),
    "l": (64, 64, 1, 50, "s0_d1", 1, 2, 8),
    "m": (3, 32, 1, 50, "s1_d1", 2, 3, 7),
    "n": (64, 64, 1, 18, D3, 4, 2, 12),
    "o": (64, 64, 1, 25, D3, 4, 2, 12),
    # residual only: projection, stride 2, odd T at V = 25, K = 2
    "r": (64, 128, 2, 25, "s1_d1", 2, 2, 13),
    # the 64 -> 128 stride-2 V = 18 block at K = 2 (distance d = 1)
    "s": (64, 128, 2, 18, "s1_d1", 2, 2, 13),
}
MATRIX = "abcdefghijklmno"
SPLIT = "acfhjn"          # unfolded split paths with K > 1, and j, which folds
BF16 = "abcefgijklo"
RESIDUAL = "akr"
NO_DX = "fk"
