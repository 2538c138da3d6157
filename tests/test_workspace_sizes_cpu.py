"""The handle-free *_workspace_bytes functions run without a GPU.  Each is a dry run of the carve its operator makes, so
it may only have shrunk against the hand count it replaced (the values of the commit before, below as literals), except where
that hand count was short of a carve a legal call can make.

Under-counts (asserted >= instead of <=):
  gp_gauss_kl_workspace_bytes      every entry: the hand count left out the item / problem / result header (768 bytes)
                                   that gauss_kl_impl carves first; it lived in the 4096-byte tail.
  gp_conditional_workspace_bytes   entries with short N: the hand count sized a float64 task, but the function also serves
                                   gp_conditional_diag_f32 / _f32w, whose carve adds two M*M/2-double copies (W, tril(Lq)^T)
                                   and saves only half of three M x N strips.
"""
import pytest

from gpitch_amd import _lib, samplecov

MS = [1, 31, 64, 96, 128, 129, 256, 320, 512, 1024]
NS = [1, 8, 255, 256, 257, 2001, 32768]

# the parent commit's values
CHOL = [1280, 39680, 98304, 172032, 262144, 265472, 786432, 1146880, 2621440, 9437184]   # gp_chol_workspace_bytes(M), M in MS
KL_WHITE = [4096, 4096, 4096, 4096, 4096, 4096, 4096, 4096, 4096, 4096]   # gp_gauss_kl_workspace_bytes(M, 0)
KL_PRIOR = [6144, 59904, 168448, 325120, 530432, 539648, 1847296, 2802176, 6852608, 26349568]   # gp_gauss_kl_workspace_bytes(M, 1)
# gp_conditional_workspace_bytes(N, M): rows N in NS, columns M in MS
COND = [
    [27904, 120832, 256512, 421888, 620032, 627968, 1740288, 2497024, 5553664, 19471872],
    [31488, 129024, 269312, 439296, 642048, 649984, 1780736, 2547456, 5631744, 19625216],
    [168704, 445184, 782080, 1148672, 1541888, 1561344, 3454720, 4607744, 8853248, 25941760],
    [169216, 445696, 782592, 1149184, 1542400, 1561856, 3455232, 4608256, 8853760, 25942272],
    [171264, 448512, 786944, 1155072, 1549824, 1570048, 3468800, 4624896, 8879616, 25992704],
    [1147136, 2680832, 4400128, 6149888, 7884032, 7987200, 15244288, 19120640, 31537664, 70415872],
    [18375936, 42061056, 68147456, 94263552, 119625984, 121206016, 222976256, 274848000, 431249664, 854087936],
]
# gp_conditional_full_workspace_bytes(N, M)
COND_FULL = [
    [29184, 122112, 257792, 423168, 621312, 629248, 1741568, 2498304, 5554944, 19473152],
    [32768, 130304, 270592, 440576, 643328, 651264, 1782016, 2548736, 5633024, 19626496],
    [171776, 448256, 785152, 1151744, 1544960, 1564416, 3457792, 4610816, 8856320, 25944832],
    [172288, 448768, 785664, 1152256, 1545472, 1564928, 3458304, 4611328, 8856832, 25945344],
    [174592, 451840, 790272, 1158400, 1553152, 1573376, 3472128, 4628224, 8882944, 25996032],
    [1164288, 2697984, 4417280, 6167040, 7901184, 8004352, 15261440, 19137792, 31554816, 70433024],
    [18639104, 42324224, 68410624, 94526720, 119889152, 121469184, 223239424, 275111168, 431512832, 854351104],
]
# gp_sgpr_predict_source_workspace_bytes(N, n): rows N in NS, columns n in NS
PREDICT_SOURCE = [
    [28160, 31744, 165376, 165888, 167424, 1115648, 17852416],
    [41984, 42496, 204288, 204800, 206336, 1350144, 21532672],
    [1602304, 1626880, 2646272, 2646784, 2656000, 10720512, 152982272],
    [1607424, 1632000, 2655488, 2655488, 2664704, 10756864, 153511168],
    [1624832, 1649408, 2680576, 2680576, 2689792, 10837248, 154576128],
    [68308736, 68502272, 76505344, 76505344, 76570368, 132852480, 1141485312],
    [17248475904, 17251650304, 17382685440, 17382689536, 17383742208, 18305243904, 34561510144],
]
# gp_conditional_workspace_bytes entries (N, M) where the float32 carve is the larger one: short N, see the docstring
COND_UNDERCOUNTED = {
    (1, 1), (1, 31), (1, 64), (1, 96), (1, 128), (1, 129), (1, 256), (1, 320), (1, 512), (1, 1024), (8, 1), (8, 31),
    (8, 64), (8, 96), (8, 128), (8, 129), (8, 256), (8, 320), (8, 512), (8, 1024), (255, 512), (255, 1024),
    (256, 512), (256, 1024), (257, 512), (257, 1024),
}
# gp_segment_gram_workspace_bytes(B, K, L): the shapes of test_kernelfit_cpu.py, then smaller ones
GRAM = {(1, 10000, 441): 18390272, (4, 10000, 441): 73560320, (1, 4, 10): 33024, (2, 7, 33): 65792, (3, 100, 64): 99840}


@pytest.fixture(scope="module")
def lib():
    return _lib.load_library()


def _check(new, old, undercounted=False, grow=0):
    assert new % 256 == 0, new
    if undercounted:
        assert old <= new <= old + grow, (new, old)
    else:
        assert new <= old, (new, old)


def test_chol_sizes(lib):
    for M, old in zip(MS, CHOL):
        _check(lib.gp_chol_workspace_bytes(M), old)


def test_gauss_kl_sizes(lib):
    for M, white, prior in zip(MS, KL_WHITE, KL_PRIOR):
        # the item, problem and result regions (256 bytes each) are now counted beside the tail, not inside it
        _check(lib.gp_gauss_kl_workspace_bytes(M, 0), white, undercounted=True, grow=768)
        _check(lib.gp_gauss_kl_workspace_bytes(M, 1), prior, undercounted=True, grow=768)


def test_conditional_sizes(lib):
    for N, row, row_full in zip(NS, COND, COND_FULL):
        for M, old, old_full in zip(MS, row, row_full):
            # the float32 carve adds two copies of M * M floats, each rounded up to 256 bytes, and halves the strips
            _check(lib.gp_conditional_workspace_bytes(N, M), old, undercounted=(N, M) in COND_UNDERCOUNTED,
                   grow=2 * ((M * M * 4 + 255) // 256 * 256))
            _check(lib.gp_conditional_full_workspace_bytes(N, M), old_full)
    assert all(N <= 257 for N, M in COND_UNDERCOUNTED)


def test_predict_source_sizes(lib):
    for N, row in zip(NS, PREDICT_SOURCE):
        for n, old in zip(NS, row):
            _check(lib.gp_sgpr_predict_source_workspace_bytes(N, n), old)
    # the window size of the benchmark: unchanged, so Windows.predict_s chunks as before
    assert lib.gp_sgpr_predict_source_workspace_bytes(2001, 2001) == PREDICT_SOURCE[NS.index(2001)][NS.index(2001)]


def test_segment_gram_sizes():
    for (B, K, L), old in GRAM.items():
        _check(samplecov.gram_workspace_bytes(B, K, L), old)


def test_degenerate_shapes_keep_their_values(lib):
    assert lib.gp_chol_workspace_bytes(0) == 256
    assert lib.gp_conditional_workspace_bytes(0, 64) == 256 and lib.gp_conditional_workspace_bytes(8, 0) == 256
    assert lib.gp_conditional_full_workspace_bytes(0, 64) == 256
    assert lib.gp_gauss_kl_workspace_bytes(0, 1) == 4096
    assert lib.gp_sgpr_predict_source_workspace_bytes(0, 5) == 256
    assert lib.gp_segment_gram_workspace_bytes(0, 1, 1) == 0
