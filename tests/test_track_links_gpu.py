"""mot_set_track_links (tests/track_link_cases.py) on the MI355X: the owner rows of csrc/track.hip against the reference's own build stepped beside
the device, the per-point ids of csrc/link.hip against the numpy composition of the getters. tests/test_emu_track_links.py runs the same bodies on
the emulator."""
import pytest

import capacity_cases as CC
import track_link_cases as LC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(mot, hip_lib):
    import hiprt

    def upload(host):
        d = hiprt.DeviceBuffer(host)
        return d.ptr, d
    return CC.Env(mot, None, upload)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_owners_against_the_reference(env, oracle, which, mode):
    streams = list(LC.golden_streams()) + [LC.crossing_stream()]
    tot = LC.owners_against_reference(env, oracle, streams[which], mode)
    if which == 2:
        assert tot["contested"] > 0, tot


@pytest.mark.parametrize("name", sorted(LC.edge_scripts()))
def test_owner_edges(env, oracle, name):
    LC.owner_edges(env, oracle, name)


def test_contested_boxes(env, oracle):
    LC.contested(env, oracle)


def test_batch_of_three(env, oracle):
    LC.batch_of_three(env, oracle)


def test_point_ids(env, oracle):
    LC.point_ids(env, oracle, LC.NE_SHAPES)


def test_point_ids_order_any(env, oracle):
    LC.order_any_equals_scan(env, oracle)


def test_point_ids_with_launch_graphs(env, oracle):
    LC.graphs_equal_plain(env, oracle)


@pytest.mark.parametrize("sequence", [False, True])
def test_persistence(env, oracle, sequence):
    LC.persistence(env, oracle, sequence)


def test_contract_links_off(env, oracle):
    LC.contract_off(env, oracle)


def test_contract_slot_taken(env, oracle):
    LC.contract_slot_taken(env, oracle)


def test_contract_refused_frame(env, oracle):
    LC.contract_refused(env, oracle)
