"""Parity away from the two presets (tests/param_cases.py) on the MI355X: grid sizes, occupancy rules, polar ranges, ground thresholds and
box-stage settings inside the declared parameter domain (include/mot.h), bit-exact against the restatement with the same constants (the
reference build has its constants compiled in, so it answers at the presets only). tests/test_emu_params.py runs the same bodies on the
emulator first."""
import pytest

import param_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(mot, hip_lib):
    import hiprt

    def upload(host):
        d = hiprt.DeviceBuffer(host)
        return d.ptr, d
    return PC.Env(mot, None, upload)


@pytest.mark.parametrize("which", ["frame", "shapes"])
@pytest.mark.parametrize("dilate", [0, 1])
@pytest.mark.parametrize("G,roi", PC.GRID_SETTINGS)
def test_grid_sizes(env, oracle, synth, G, roi, dilate, which):
    PC.grid_case(env, oracle, synth, G, roi, dilate, which)


def test_grid_256_with_labels_only(env, oracle, synth):
    PC.grid_case(env, oracle, synth, 256, 50.0, 1, "frame", flags=(PC.OUT_LABELS,))


@pytest.mark.parametrize("occ,dilate", [(1, 0), (1, 1), (2, 0), (2, 1)])
def test_occupancy_rule(env, oracle, synth, occ, dilate):
    PC.occupancy_case(env, oracle, synth, occ, dilate)


@pytest.mark.parametrize("r_min,r_max", PC.POLAR_RANGES)
def test_polar_range(env, oracle, synth, r_min, r_max):
    PC.polar_case(env, oracle, synth, r_min, r_max)


@pytest.mark.parametrize("over", PC.GROUND_SETTINGS, ids=PC.ident)
def test_ground_thresholds(env, oracle, synth, over):
    PC.ground_case(env, oracle, synth, over)


@pytest.mark.parametrize("over", PC.BOX_SETTINGS, ids=PC.ident)
def test_box_stage(env, oracle, synth, over):
    PC.box_case(env, oracle, synth, over)


@pytest.mark.parametrize("along_y", [False, True])
def test_one_cluster_over_the_whole_picture(env, oracle, synth, along_y):
    PC.box_wide_case(env, oracle, synth, along_y)


@pytest.mark.parametrize("preset,over,kind", PC.track_pairs(), ids=lambda v: PC.ident(v) if isinstance(v, dict) else str(v))
def test_tracker_thresholds(env, oracle, preset, over, kind):
    PC.tracker_case(env, oracle, preset, over, kind)
