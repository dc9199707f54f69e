"""GPU parity of k_searchN (csrc/track.hip) at the counts where its trips split: windows of 0, 1, N - 1, N, N + 1, 2 N and 2 N + 1 corners
(N = 128 corners per lane group and filter trip), 0, 1, K - 1, K, K + 1 and 2 K + 1 survivors (K = 4 candidates scored per trip), an empty
window, a survivor that fails the border test in the middle of a trip, two candidates of equal best ZMSSD in one trip and in two (the
earlier in raster order wins), and one wavefront whose patches mix the extremes.  The cases come from tests/search_trip_cases.py;
tests/test_search_trip_cases.py asserts on the CPU that the oracle reaches every count.  Here every case is a stream of one System
beside its own oracle (stagewise.run_group): searched and found sets, vfound, image, attempted, found and n_zmssd are
compared with == after each search and pose stage, then the frame through helpers.assert_tracker_exact; two frames per case, the second
on the cached templates."""
import pytest

import search_trip_cases as sc
from stagewise import run_group

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("patch", [8, 11])
@pytest.mark.parametrize("group", sc.GROUP_NAMES)
def test_search_at_every_trip_count(group, patch):
    """batches of 17, 9 and 1 streams (xcd_stream_block's third, second and first group of eight)"""
    cases = sc.groups(patch)[group]
    assert len(cases) in (1, 9, 17)
    run_group(cases, patch)
