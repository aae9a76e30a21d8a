"""Self-test of the float64 references and operand builders of tests/tn_cases.py (no GPU): the references against torch's own operators and
against each other on tiny shapes, the claimed f16 -> bf16 roundings, and the exactness precondition of every EXACT operand set that
tests/test_tn_blocks_gpu.py builds (through the same builders; the long-K sets by formula)."""
import pytest
import torch

from tests import nt_epilogue_cases as C
from tests import tn_cases as T


@pytest.mark.parametrize("lgS", [4, 5])
@pytest.mark.parametrize("regime", ["exact", "real"])
def test_conv_wgrad_ref_is_torchs_conv2d_weight(regime, lgS):
    S = 1 << lgS
    dy_pad, x_pad = T.conv_case(regime, 2, lgS, 4, 8, 5)
    assert bool(torch.isnan(dy_pad[:, 0].float()).all()) and not bool(x_pad[:, 0].float().abs().any())
    got = T.conv_wgrad_ref(dy_pad, x_pad, lgS).view(8, 3, 3, 4).permute(0, 3, 1, 2)
    x = x_pad[:, 1:S + 1, 1:S + 1].double().permute(0, 3, 1, 2)
    dy = dy_pad[:, 1:S + 1, 1:S + 1].double().permute(0, 3, 1, 2)
    ref = torch.nn.grad.conv2d_weight(x, (8, 4, 3, 3), dy, padding=1)
    assert float((got - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    if regime == "exact":
        assert torch.equal(got, ref)


def test_unpool_rows_is_the_routing_of_the_pooling():
    """tests/test_gemm_gpu.py states the routing on the image: the value stands at pixel (2 py + q / 2, 2 px + q % 2) of its window where the
    byte is q, nothing where it is 4 (or above)."""
    P, Cc = 2, 8
    g = torch.Generator().manual_seed(3)
    dy = torch.randn(P * 64, Cc, generator=g)
    code = T.codes((P * 64, Cc), 4)
    assert bool((code > 4).any()) and all(bool((code == q).any()) for q in range(5))
    img = torch.zeros(P, 16, 16, Cc)
    dyc, cc = dy.view(P, 8, 8, Cc), code.view(P, 8, 8, Cc)
    for q in range(4):
        img[:, (q >> 1)::2, (q & 1)::2] = torch.where(cc == q, dyc, torch.zeros(()))
    yy, xx = C.window_major(16)
    assert torch.equal(T.unpool_rows(dy, code), img[:, yy, xx].reshape(P * 256, Cc))


@pytest.mark.parametrize("regime", ["exact", "real"])
def test_list_ref_on_the_identity_list_is_the_convolution_of_the_unpooled_maps(regime):
    c = T.conv3_pairs_case(regime, 2, 7)
    got = T.list_wgrad_ref(c["dy"], c["code"], c["gather"], c["dest"], c["z"])
    ref = T.conv_wgrad_ref(T.unpooled_pad(c), c["z"], 4)
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()) and float(ref.abs().max()) > 0
    if regime == "exact":
        assert torch.equal(got, ref)


def test_list_ref_with_duplicates_and_a_permutation_is_the_sum_of_its_entries():
    c = T.list_case("exact", 16, 21)
    ga, de = c["gather"], c["dest"]
    assert ga.unique().numel() < 16 and de.unique().numel() < 16 and bool((ga[1:] < ga[:-1]).any())
    for w in (0, 7, 56, 63, 5 * 64, 5 * 64 + 7, 5 * 64 + 56, 5 * 64 + 63):
        assert w in ga.tolist()
    whole = T.list_wgrad_ref(c["dy"], c["code"], ga, de, c["z"])
    perm = torch.randperm(16, generator=torch.Generator().manual_seed(1))
    assert torch.equal(T.list_wgrad_ref(c["dy"], c["code"], ga[perm], de[perm], c["z"]), whole)
    parts = sum(T.list_wgrad_ref(c["dy"], c["code"], ga[e:e + 1], de[e:e + 1], c["z"]) for e in range(16))
    assert torch.equal(parts, whole)
    # the dead window (all codes 4) gives nothing although its gradient row is not zero; the im2col rows state the same product
    assert not bool(T.list_wgrad_ref(c["dy"], c["code"], ga[8:9], de[8:9], c["z"]).any())
    dy3x = T.unpool_rows(c["dy"][de.long()], c["code"][ga.long()])
    assert torch.equal(T.tn_ref(dy3x, T.zcol_rows(ga, c["z"])), whole)


def test_f16_integers_round_to_bf16_as_claimed():
    z = torch.tensor(T.F16_TIES, dtype=torch.float16)
    assert z.tolist() == list(T.F16_TIES)                                      # f16 holds them
    assert z.to(torch.bfloat16).tolist() == [260, 260, 264, 520, 2048]
    assert z.float().view(torch.int32).bitwise_and(-65536).view(torch.float32).tolist() == [258, 260, 262, 516, 2040]     # truncation differs


def test_expected_slabs():
    assert [T.expected_slabs(5, s, 3) for s in (1, 2, 4, 9)] == [1, 2, 3, 5]
    assert T.expected_slabs(20, 3, 72) == 3 and T.expected_slabs(1, 32, 32) == 1 and T.expected_slabs(5, 32, 32) == 5
    assert T.expected_slabs(2053, -1, 72, sparse=True) == 32 and T.expected_slabs(2048, -1, 72, sparse=True) == 32
    assert T.expected_slabs(2047, -1, 72, sparse=True) == T.expected_slabs(2047, 0, 72) == 7
    assert T.expected_slabs(16, 0, 10) == 2 and T.expected_slabs(4, 0, 72) == 1 and T.expected_slabs(8194, 0, 72) == 7


# ---- the exactness precondition of every EXACT operand set of the GPU file
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_exact_plain_sets(dtype):
    for i, (M, N, K, _) in enumerate(T.PLAIN_STRIDED + T.PLAIN_SIZE_RULE + T.PLAIN_WALK):
        if (M, N) == (4096, 2560) and dtype == torch.float16:
            continue                                                            # same draws in both types: one is enough for the largest
        A, B = T.plain_case("exact", K, M, N, dtype, 100 + i)
        C.assert_exact(A, B, mag=T.tn_ref(A.abs(), B.abs()))
    for XC, n_rows, _ in T.CONV1:
        A, B = T.plain_case("exact", n_rows, 128, XC, torch.bfloat16, 200)
        C.assert_exact(A, B, mag=T.tn_ref(A.abs(), B.abs()))
    for n_rows, _ in T.FC2:
        A, B = T.plain_case("exact", n_rows, 512, 4096, torch.bfloat16, 210)
        C.assert_exact(A, B, mag=T.tn_ref(A.abs(), B.abs()))
    for n_rows, cols in T.FC1:
        A, B = T.plain_case("exact", n_rows, 4096, cols, torch.bfloat16, 220)
        C.assert_exact(A, B, mag=T.tn_ref(A.abs(), B.abs()))


def test_exact_conv_sets():
    for n, lgS, Cin, M, _ in T.CONV_DBG:
        dy, x = T.conv_case("exact", n, lgS, Cin, M, 300)
        C.assert_exact(dy[:, 1:-1, 1:-1], x, mag=T.conv_wgrad_ref(dy.abs(), x.abs(), lgS))
    for n_obj in sorted({n for n, _ in T.CONV2}):
        dy, x = T.conv_case("exact", n_obj, 5, 128, 512, 310)
        C.assert_exact(dy[:, 1:-1, 1:-1], x, mag=T.conv_wgrad_ref(dy.abs(), x.abs(), 5))
    for P, _ in T.CONV3:
        c = T.conv3_pairs_case("exact", P, 320 + P)
        C.assert_exact(c["dy"], c["z"], mag=T.list_mag(c))


def test_exact_list_sets():
    for E in sorted({r // 4 for r in T.LIST_ROWS} | {e for e, _ in T.SPARSE_ENTRIES}):
        c = T.list_case("exact", E, 400 + E)
        C.assert_exact(c["dy"], c["z"], mag=T.list_mag(c))
        c = T.list_case("exact", E, 500 + E, z_dtype=torch.float16, z_values=T.F16_TIES + (257, 300, 1025, 1999))
        assert not torch.equal(c["z"].to(torch.bfloat16).float(), c["z"].float())                # the conversion rounds
        m = T.list_mag(dict(c, z=c["z"].to(torch.bfloat16)))
        C.assert_exact(c["dy"], c["z"], mag=m)


def test_exact_grouped_set_on_its_largest_group():
    c = T.grouped_case("exact", 600)
    sizes = T.group_sizes()
    assert sizes[0] == 0 and sizes[63] == 0 and set(sizes) == set(T.GROUP_CYCLE) and c["rows"] == sum(sizes)
    g = sizes.index(320)
    g0 = int(c["goff"][g])
    A, B = c["gwm"][g0:g0 + 320], c["ywm"][g0:g0 + 320]
    C.assert_exact(A, B, mag=T.tn_ref(A.abs(), B.abs()))
    assert 320 * 9 < 2 ** 24                                                    # every group: at most 320 products of at most 3 * 3


def test_exact_long_sets_by_formula():
    c = T.long_list_case(256, 700)
    T.long_exact(c, max(T.LONG_ENTRIES))                                        # one product per entry and output element
    T.long_exact(c, T.LONG_PAIRS * 64)
    T.long_exact(c, 131072 + 32)
    assert torch.equal(c["z"].to(torch.bfloat16).float(), c["z"].float())       # these maps convert without rounding
    m = T.list_mag(c)                                                           # and on a slice, against the formula's bound
    assert float(m.max()) <= 256 * 9
