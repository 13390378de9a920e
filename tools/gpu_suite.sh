#!/bin/bash
source tools/gpu_guard.sh
export TMPDIR=/tmp
O=gpurun_out/${1:-r05suite}; mkdir -p $O
# K1's lockstep rounds, its window order and its claimed tail first, alone, under a short limit
# of their own: a miscounted barrier hangs, and after a hang nothing else may
# start.  No per-test --timeout here: pytest-timeout would end a hung test with exit
# status 1, which looks like an ordinary failure; only the outer limit
# applies, so a hang ends as 124.  And this step is fatal on any status but 0
# (not through the guard's run, which goes on after an ordinary failure): the
# suite does not start on a K1 that hung, faulted or miscounted.
timeout -k 10 300 python -u -m pytest tests/test_gpu_k1_order.py tests/test_gpu_k1_lockstep.py tests/test_gpu_k1_tail.py -q -m gpu -p no:cacheprovider -p no:timeout > $O/pytest_k1_lockstep.log 2>&1
rc=$?
echo "[step rc=$rc] tests/test_gpu_k1_order.py tests/test_gpu_k1_lockstep.py tests/test_gpu_k1_tail.py" >&2
tail -1 $O/pytest_k1_lockstep.log
[ $rc -eq 0 ] || { echo "[guard] K1 lockstep step rc=$rc, stopping" >&2; exit $rc; }
run 900 python -u -m pytest tests -q -m gpu --timeout 120 --timeout-method thread -p no:cacheprovider > $O/pytest.log 2>&1
tail -1 $O/pytest.log
run 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1
echo done
