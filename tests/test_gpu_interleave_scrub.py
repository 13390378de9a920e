"""crc32c_scrub_pages among the other entry points, out of order: the ops of
tests/scrub_interleave_cases.py are mixed into an order of
tests/interleave_cases.py's table, run directly behind every call that returned
early, and the scrub call's own early returns are followed by every call that
succeeds.  Every run is compared exactly with its op's expectation.  All calls
of a process share the Device's grow-only scratch; the scrub call uses that of
the three calls it composes, whole-list recover scratch and a few buffers of
its own."""
import pytest

try:  # GPU processes load torch (and its HIP runtime) before libmcrc32c.so
    import torch as _torch  # noqa: F401
except ImportError:
    pass

from . import interleave_cases as ic
from . import raw_calls
from . import scrub_interleave_cases as sic

pytestmark = pytest.mark.gpu
SCRUB_OPS = sic.table()
ERROR_OPS = [op for op in SCRUB_OPS if op.error]
GOOD_OPS = [op for op in SCRUB_OPS if not op.error]


@pytest.fixture(scope="module")
def torch():
    return raw_calls.need_gpu()


def _run_and_check(torch, op, tag=""):
    with raw_calls.small_max(op.small_max):
        got = op.run(torch, None)
    ic.check(op, got, tag)


@pytest.mark.parametrize("order", ["seed2", "largest_first"])
def test_scrub_calls_inside_the_tables_orders(torch, order):
    """The table's order with a scrub op put in behind every third op, in turn;
    behind each error op comes a different entry point that succeeds
    (ic.separate_errors)."""
    ops, k = [], 0
    for j, op in enumerate(ic.orders()[order]):
        ops.append(op)
        if j % 3 == 2:
            ops.append(SCRUB_OPS[k % len(SCRUB_OPS)])
            k += 1
    ops = ic.separate_errors(ops)
    assert k >= len(SCRUB_OPS)
    for j, op in enumerate(ops):
        _run_and_check(torch, op, tag=f"{order}[{j}] after {ops[j - 1].name if j else 'nothing'}")


def test_scrub_calls_after_every_error(torch):
    """Each scrub op directly behind each call of the table that returned
    early, which is checked every time as well."""
    for err in ic.error_ops():
        for op in GOOD_OPS:
            _run_and_check(torch, err, tag=f"before {op.name}")
            _run_and_check(torch, op, tag=f"after {err.name}")


def test_every_op_after_the_scrub_calls_early_returns(torch):
    """Each call that succeeds, the scrub ops among them, directly behind a
    scrub call that returned early."""
    for err in ERROR_OPS:
        for op in list(ic.success_ops()) + GOOD_OPS:
            _run_and_check(torch, err, tag=f"before {op.name}")
            _run_and_check(torch, op, tag=f"after {err.name}")
