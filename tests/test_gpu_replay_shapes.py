"""The run-time shapes of the exact-set dedup tail (replay_lds.hip, partition.h) give the same tables: the default, and partition
tiles / scatter stages of other sizes (a stage smaller than a tile sends the rest of the tile's pairs out directly)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = {
    "default": {},
    "lean_tile8_stage2048": {"SYLPH_HIP_PART_TILE_BLOCKS": "8", "SYLPH_HIP_PART_STAGE_PAIRS": "2048"},
    "lean_stage256": {"SYLPH_HIP_PART_STAGE_PAIRS": "256"},
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_replay_shapes_match_the_oracle(shape):
    env = dict(os.environ)
    for k in ("SYLPH_HIP_PART_TILE_BLOCKS", "SYLPH_HIP_PART_STAGE_PAIRS"):
        env.pop(k, None)
    env.update(SHAPES[shape])
    r = subprocess.run([sys.executable, "-m", "tests.replay_shapes_worker"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "replay shapes ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
