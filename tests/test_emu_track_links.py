"""mot_set_track_links (tests/track_link_cases.py) on the emulator: the owner rows of csrc/track.hip, the per-point kernel of csrc/link.hip and the host
layer around them. The same bodies run on the MI355X in tests/test_track_links_gpu.py. The oracle tracker is the reference's own build where
oracle/_ref is on the box (oracle_lib.RefFirst), the C restatement otherwise."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import capacity_cases as CC
import track_link_cases as LC


@pytest.fixture(scope="module")
def env(mot):
    import build_emu
    return CC.Env(mot, build_emu.build())


@pytest.fixture
def ref_first(oracle):
    return oracle.RefFirst(oracle) if oracle.ref() is not None else oracle


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_emu_owners_against_the_reference(env, ref_first, which, mode):
    streams = list(LC.golden_streams()) + [LC.crossing_stream()]
    tot = LC.owners_against_reference(env, ref_first, streams[which], mode)
    if which == 2:
        assert tot["contested"] > 0, tot   # neighbouring gates do share boxes on the 2 m lattice


@pytest.mark.parametrize("name", sorted(LC.edge_scripts()))
def test_emu_owner_edges(env, oracle, name):
    LC.owner_edges(env, oracle, name)


def test_emu_contested_boxes(env, oracle):
    LC.contested(env, oracle)


def test_emu_batch_of_three(env, oracle):
    LC.batch_of_three(env, oracle)


def test_emu_point_ids(env, oracle):
    LC.point_ids(env, oracle, LC.NE_SHAPES)


def test_emu_point_ids_order_any(env, oracle):
    LC.order_any_equals_scan(env, oracle)


def test_emu_point_ids_with_launch_graphs(env, oracle):
    LC.graphs_equal_plain(env, oracle)


@pytest.mark.parametrize("sequence", [False, True])
def test_emu_persistence(env, oracle, sequence):
    LC.persistence(env, oracle, sequence)


def test_emu_contract_links_off(env, oracle):
    LC.contract_off(env, oracle)


def test_emu_contract_slot_taken(env, oracle):
    LC.contract_slot_taken(env, oracle)


def test_emu_contract_refused_frame(env, oracle):
    LC.contract_refused(env, oracle)


def test_emu_link_kernel_launched_only_with_links_on(env, oracle):
    lib = env.mot.load_library(env.lib_path)
    count = lambda: lib.hipemu_launch_count(b"point_tracks_kernel")
    with env.context(0, max_points=4096, max_tracks_total=256) as c:
        before = count()
        LC.launch(env, c, [CC.small_scene(0, 12)], 4096, 0)
        assert count() == before
        c.set_track_links(True)
        LC.launch(env, c, [CC.small_scene(1, 12)], 4096, 1)
        assert count() == before + 1
