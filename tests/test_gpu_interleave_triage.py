"""crc32c_triage_pages among the other entry points, out of order: the ops of
tests/triage_interleave_cases.py are mixed into an order of
tests/interleave_cases.py's table, run directly behind every call that returned
early, and the triage call's own early return (CRC32C_EWORK behind the scan) is
followed by every call that succeeds.  Every run is compared exactly with its
op's expectation.  All calls of a process share the Device's grow-only scratch;
the triage call uses crc32c_recover_pages' and two buffers of its own."""
import pytest

try:  # GPU processes load torch (and its HIP runtime) before libmcrc32c.so
    import torch as _torch  # noqa: F401
except ImportError:
    pass

from . import interleave_cases as ic
from . import raw_calls
from . import triage_interleave_cases as tic

pytestmark = pytest.mark.gpu
TRIAGE_OPS = tic.table()
EWORK_OP = TRIAGE_OPS[-1]
GOOD_OPS = TRIAGE_OPS[:-1]


@pytest.fixture(scope="module")
def torch():
    return raw_calls.need_gpu()


def _run_and_check(torch, op, tag=""):
    with raw_calls.small_max(op.small_max):
        got = op.run(torch, None)
    ic.check(op, got, tag)


@pytest.mark.parametrize("order", ["seed2", "largest_first"])
def test_triage_calls_inside_the_tables_orders(torch, order):
    """The table's order with a triage op put in behind every third op, the six
    in turn; behind each error op comes a different entry point that succeeds
    (ic.separate_errors)."""
    ops, k = [], 0
    for j, op in enumerate(ic.orders()[order]):
        ops.append(op)
        if j % 3 == 2:
            ops.append(TRIAGE_OPS[k % len(TRIAGE_OPS)])
            k += 1
    ops = ic.separate_errors(ops)
    assert k >= 2 * len(TRIAGE_OPS)
    for j, op in enumerate(ops):
        _run_and_check(torch, op, tag=f"{order}[{j}] after {ops[j - 1].name if j else 'nothing'}")


def test_triage_calls_after_every_error(torch):
    """Each triage op directly behind each call of the table that returned
    early, which is checked every time as well."""
    assert EWORK_OP.error and not any(op.error for op in GOOD_OPS)
    for err in ic.error_ops():
        for op in GOOD_OPS:
            _run_and_check(torch, err, tag=f"before {op.name}")
            _run_and_check(torch, op, tag=f"after {err.name}")


def test_every_op_after_the_triage_calls_early_return(torch):
    """Each call that succeeds, the triage ops among them, directly behind a
    triage call that returned CRC32C_EWORK."""
    for op in list(ic.success_ops()) + list(GOOD_OPS):
        _run_and_check(torch, EWORK_OP, tag=f"before {op.name}")
        _run_and_check(torch, op, tag=f"after {EWORK_OP.name}")
