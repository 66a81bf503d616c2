"""The per-frame capacity edges of the cluster and box stage (tests/capacity_cases.py) on the MI355X: at each limit bit-exact against the
oracle (the reference build answers first), one beyond it a plain MOT_E_CAPACITY from kernels that stay inside their buffers, and the
contract after a refusal. tests/test_emu_capacity.py runs the same bodies under the emulator's AddressSanitizer build FIRST
(tests/README.md, "capacity edges"): nothing here relies on a fault."""
import pytest

import capacity_cases as CC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(mot, hip_lib):
    import hiprt

    def upload(host):
        d = hiprt.DeviceBuffer(host)
        return d.ptr, d
    return CC.Env(mot, None, upload)


@pytest.mark.parametrize("max_points,permuted", [(8192, False), (12288, True)])
def test_group_edge_stagewise(env, oracle, max_points, permuted):
    CC.groups_stagewise(env, oracle, max_points, permuted)


def test_refused_frame_finds_nothing_of_an_earlier_frame(env, oracle):
    CC.groups_refused_first(env, oracle)


def test_cluster_edge_stagewise(env, oracle):
    CC.clusters_stagewise(env, oracle)


def test_box_edge_stagewise(env, oracle):
    CC.boxes_stagewise(env, oracle)


@pytest.mark.parametrize("kind,graphs", [("groups", False), ("groups", True), ("clusters", False), ("boxes", False)])
def test_fused_refusal_contract(env, oracle, kind, graphs):
    CC.fused_contract(env, oracle, kind, graphs)


def test_sequence_mode_reports_a_refused_frame(env, oracle):
    CC.sequence_refusal(env, oracle)


def test_ram_points_edge(env, oracle):
    CC.ram_points_edge(env, oracle)
