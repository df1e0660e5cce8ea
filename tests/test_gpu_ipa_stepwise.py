"""gm_ipa_new against tests/stepwise/ipa.py, the literal composition of the per-prover entry points the suite already covers
(gm_sc_*, gm_hg1_*, gm_hg2_*, gm_hp_*, gm_pairing_multi, gm_gt_mul / gm_gt_pow): the same bytes in every field and the same
transcript afterwards.  This pins the batched fold and the segmented Miller product to the per-prover kernels."""
import numpy as np
import pytest

from gemini_amd.g2msm import g2_points_to_affine
from tests import ipa_exponent_ref as X
from tests.stepwise import ipa as steps
from tests.test_gpu_ipa import LABEL, mont, scalars
from tests.test_gpu_pairing import g1_points_to_affine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


@pytest.mark.parametrize("d,n", [(8, 16), (64, 128)])
def test_same_bytes_as_the_per_prover_composition(gm, d, n):
    p1, _, p2, _ = X.crs(n)
    a, b = scalars(3000 + d, d), scalars(4000 + d, d)
    t_steps, t_lib = gm.Transcript(LABEL), gm.Transcript(LABEL)
    exp = steps.new(t_steps, p1, p2, a, b)
    crs = gm.Crs(g1_points_to_affine(p1), g2_points_to_affine(p2))
    proof = gm.InnerProductProof.new(t_lib, crs, mont(a), mont(b))
    f = proof.fields()
    assert f.rounds == exp["rounds"] == X.ceil_log2(d)
    assert f.messages.tobytes() == exp["messages"].tobytes()
    assert f.challenges.tobytes() == np.stack(exp["challenges"]).tobytes()
    assert f.batch_challenges.tobytes() == np.stack(exp["batch_challenges"]).tobytes()
    assert len(exp["final_foldings"]) == 2 * (f.rounds - 1)
    for p, (l, r) in enumerate(exp["final_foldings"]):
        assert f.final_lhs[p].tobytes() == l.tobytes() and f.final_rhs[p].tobytes() == r.tobytes(), p
    assert f.foldings_ff.tobytes() == np.stack(exp["foldings_ff"]).tobytes()
    assert f.foldings_fg1[0].tobytes() == exp["foldings_fg1"][0].tobytes() and f.foldings_fg1[1].tobytes() == exp["foldings_fg1"][1].tobytes()
    assert f.foldings_fg2[0].tobytes() == exp["foldings_fg2"][0].tobytes() and f.foldings_fg2[1].tobytes() == exp["foldings_fg2"][1].tobytes()
    assert t_lib.challenge_bytes(b"next", 32) == t_steps.challenge_bytes(b"next", 32)
    for o in (proof, crs, t_lib, t_steps):
        o.free()
