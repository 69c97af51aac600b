"""Grid size never changes what the chunk-indexed decoder computes, on the real kernels (run with `pytest -m gpu` on an MI355X; tests/test_dx_grid_emulated.py runs the
same bodies on the emulated product and pins the kernels' coefficients on the CPU).

k_dec_index, k_dec_reindex and k_dec_tiles are persistent grid-stride kernels whose grids the library sizes by what else is in flight.  With one
workgroup every wave walks chunk after chunk and tile after tile, with seven the work is no multiple of the grid, and the library's own shape has more workgroups than
these small inputs have work: the samples and the YUY2 pictures of the 4-frame 320 x 192 batch and the pictures of two hand-made samples are byte-identical under
all three, and what the first setting gives is checked against the oracle."""
import pytest
import dx_grid as D

pytestmark = pytest.mark.gpu


def test_batch_samples_and_pictures_are_the_same_under_every_grid():
    own = D.batch_round_trip(None)
    D.check_batch(own[0], own[1], "the library's own grids")
    for grid in (1, 7):
        D.same_batches(D.batch_round_trip(grid), own, "%d workgroups against the library's own grids" % grid)


@pytest.mark.parametrize("name", ["mixed", "full_tile"])
def test_hand_made_pictures_are_the_same_under_every_grid(name):
    D.check_hand_made(name, (None, 1, 7))
