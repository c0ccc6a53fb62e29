"""Row passes that run on the column waves DURING the convolution in the fused lifting kernel's fp16 form (eqa_lift5_fft48k5_input_f16x2,
FORM 2 of csrc/lift_fft.hip: lf_h2_rowmask says which wave transforms which four tile rows in which sub-phase or in the tail).

While a column wave transforms rows of the item being convolved it still holds the spectrum of the PREVIOUS item in registers, waiting
for its stores.  The launches of tests/test_gpu_lift_conv_dealing.py have at most as many items as blocks
(nblk = min((256 / ngrp) * ngrp, nwork)): no wave there ever holds a pending item beside a row pass.  Here blocks run two items, and
the drain iteration (columns and stores only) follows a real one.  What can go wrong:

  * a pass that clobbers the pending registers corrupts the previous item's spectrum (another tile of V, whole frequencies);
  * a pass in front of the barrier its rows' convolution sits behind transforms rows that are not written yet, or the previous item's;
  * a pass skipped, or run twice (the transform is in place: twice is not once).

Each is an error of the size of the data in whole rows or whole frequencies, where a rounding change is of order 1e-7.  Reference, bound
and images are those of tests/test_gpu_lift_conv_dealing.py: the whole of V against the fp64 evaluation carried through torch.fft, no
further from it than the fp32 form, NaN behind the input buffer; random images and images constant along each row with a different
value per row."""
import pytest
import torch

from test_gpu_lift_conv_dealing import _check, _images  # noqa: F401  (_images: what `kind` selects inside _check)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda:0")


# (nimg, H0, W0, C)
# A: 17 tiles x 16 groups = 272 items on 256 blocks: the smallest launch in which blocks run two items (16 of them) and the drain
#    iteration follows a real one
# B: the headline's 2 x 2 tile grid, 320 items on 256 blocks
# C: ragged right and bottom edges in every sub-phase, 320 items
# D: one item per block (16 items): no pending item beside any pass
SHAPES = [(17, 52, 52, 256), (5, 96, 96, 256), (5, 57, 53, 256), (2, 96, 96, 32)]


def test_shapes_put_a_pending_item_beside_the_row_passes():
    """The launch rule of csrc/lift_fft.hip (one block per CU, a multiple of the group count): A..C run more items than blocks."""
    from equiadapt_amd.images.canonicalization_networks import fftconv

    for (nimg, H0, W0, C), two in zip(SHAPES, (True, True, True, False)):
        ngrp = C // 16
        nwork = nimg * fftconv.tiles(H0 - 4) * fftconv.tiles(W0 - 4) * ngrp
        nblk = min((256 // ngrp) * ngrp, nwork)
        assert (nwork > nblk) == two and nwork <= 2 * nblk, (nimg, H0, W0, C, nwork, nblk)


@pytest.mark.parametrize("relu_bias", [True, False], ids=["relu_bias", "plain"])
@pytest.mark.parametrize("nimg,H0,W0,C", SHAPES)
@pytest.mark.parametrize("kind", ["random", "rows"])
def test_row_passes_beside_a_pending_item_leave_both_items_whole(dev, kind, nimg, H0, W0, C, relu_bias):
    _check(dev, kind, nimg, H0, W0, C, relu_bias, relu_bias)
