"""CPU (oracle): why tests/test_gpu_small_row_sets.py adds points to the smoke scene.  Neither the scene of __graft_entry__.smoke()
(4 frames) nor its 8-frame form has a min_count that leaves exactly 3 or exactly 5 rows: the best counts tie."""
import numpy as np
import pytest

import scenes


@pytest.mark.parametrize("n_frames", [4, 8])
def test_no_min_count_leaves_three_or_five_rows(oracle_mod, synth_mod, n_frames):
    sc = scenes.Scene(n_frames, 160, 120, 0.001, fx=615.0, clean_every=2)
    og = oracle_mod.OracleGrid(resolution=sc.resolution, bbox=sc.bbox)
    c = np.sort(scenes.run(og, sc, "capture")["count"])[::-1].astype(np.int64)
    print("%d frames: best counts %s" % (n_frames, c[:8]))
    assert c[2] == c[3] and c[4] == c[5], c[:8]
