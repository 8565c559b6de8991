"""The refusals of the sequential Monte Carlo wrappers that sit behind the GPU check -- shapes, devices, the layout of
loglik_in / ll_cur / x_next / aux_*, horizons, the values of aux_sel -- against the recorded table
tests/golden/smc_refusals.json (tests/smc_refusals_util.py): the exception's class and its whole message.  K = C = 2,
N = 64, T = 8; every case refuses before a launch, so no kernel starts."""
import pytest

from tests import smc_refusals_util as U

pytestmark = pytest.mark.gpu
CASES = U.load_table()["gpu"]


def test_table_holds_every_case():
    strip = lambda c: {k: v for k, v in c.items() if k not in ("class", "message")}
    dumps = lambda cases: U.json.dumps(cases, sort_keys=True)      # NaN arguments compare as text
    assert dumps([strip(c) for c in CASES]) == dumps(U.gpu_cases())


@pytest.mark.parametrize("case", CASES, ids=U.case_id)
def test_refusal(case):
    e = U.run_case(case, "cuda:0")
    assert type(e).__name__ == case["class"] and str(e) == case["message"]
