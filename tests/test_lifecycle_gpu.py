"""A context's life cycle on the MI355X (tests/lifecycle_cases.py): create -> every lazily allocating path of the ABI once -> destroy, three times in one
process. Every call is a valid one and returns MOT_OK; what the rounds read — the boxes of every frame, the tracks of both streams — is the same bytes in
every round, the boxes are the oracle's for those frames bit for bit and the tracks the oracle tracker's. No assertion on free device memory (the machines
are shared): that nothing is left behind is what tests/test_emu_lifecycle.py counts on the emulator."""
import pytest

import capacity_cases as CC
import lifecycle_cases as LC

pytestmark = pytest.mark.gpu


def test_three_contexts_in_a_row_compute_the_same_and_what_the_oracle_computes(mot, hip_lib, oracle):
    env = CC.Env(mot)   # (host ingest only: no device pointer is handed in)
    frames = LC.clouds()
    runs = []
    for _ in range(3):
        with LC.context(env) as c:
            runs.append(LC.touch_everything(env, c, frames))
    first = LC.flatten(runs[0][0], runs[0][1])
    for k in (1, 2):
        LC.same_run(LC.flatten(runs[k][0], runs[k][1]), first, ("round", k))
    LC.against_oracle(oracle, *runs[0])
