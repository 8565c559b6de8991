"""Every refusal of the sequential Monte Carlo wrappers that CPU tensors reach -- the eleven ops functions from
sde_simulate to sv_cpmmh (and cpm_fresh_aux) and the six particle methods of PosteriorDiagnostics on a stub -- against
the recorded table tests/golden/smc_refusals.json (tests/smc_refusals_util.py): the exception's class and its whole
message.  The cases with two bad arguments pin which refusal comes first, the GPU check among them."""
import pytest

from tests import smc_refusals_util as U

CASES = U.load_table()["host"]


def test_table_holds_every_case():
    """The table is the generator's case list, in its order: no case was dropped from either."""
    strip = lambda c: {k: v for k, v in c.items() if k not in ("class", "message")}
    dumps = lambda cases: U.json.dumps(cases, sort_keys=True)      # NaN arguments compare as text
    assert dumps([strip(c) for c in CASES]) == dumps(U.host_cases())


@pytest.mark.parametrize("case", CASES, ids=U.case_id)
def test_refusal(case):
    e = U.run_case(case, "cpu")
    assert type(e).__name__ == case["class"] and str(e) == case["message"]
