"""The host side of traces enqueued ahead, without a GPU: what TrainStep.__call__ enqueues (training/step.py:plan_ahead) and
how ops.trace_rays reads its round counters (which chunks go on, the next round guess)."""
import pytest
import torch

from nefii_amd import _lib, ops
from nefii_amd.training.step import plan_ahead

a, b, c, d, e, f, g, h, x = (object() for _ in range(9))


@pytest.mark.parametrize('queued,current,upcoming,group,cur_iter,keep,own_first,calls', [
    ([], a, [b, c, d], 1, 10, True, True, [([b], [11]), ([c], [12]), ([d], [13])]),
    ([b, c, d], b, [c, d, e], 1, 11, True, False, [([e], [14])]),
    ([b, c, d], b, x, 1, 11, False, True, [([x], [12])]),       # a single input with more in flight: a change of plan
    ([], a, [b, c, d, e, f, g, h], 4, 10, True, True, [([b, c, d, e], [11, 12, 13, 14])]),
    ([], a, [b, c], 4, 10, True, True, [([b, c], [11, 12])]),       # the queue must not run dry
    ([b], b, [c, d], 4, 11, True, False, [([c, d], [12, 13])]),
    ([b, c], b, [c, d, e], 4, 11, True, False, []),                 # a traced batch is left for the next call: wait for a whole group
])
def test_plan_ahead(queued, current, upcoming, group, cur_iter, keep, own_first, calls):
    got_keep, got_own, got = plan_ahead(queued, current, upcoming, group, cur_iter)
    assert (got_keep, got_own) == (keep, own_first)
    assert len(got) == len(calls)
    for (inputs, iterations), (want_inputs, want_iterations) in zip(got, calls):
        assert len(inputs) == len(want_inputs) and all(p is q for p, q in zip(inputs, want_inputs))
        assert list(iterations) == want_iterations


def test_round_counters_name_the_chunks_with_work_and_the_next_guess():
    cnt = torch.zeros(2, 6, _lib.TRACE_COUNTERS, dtype=torch.int32)
    assert ops._next_guess(cnt) == 3
    cnt[1, 3, _lib.CNT_WORK[1]] = 5
    assert ops._chunks_with_work(cnt, 4) == [1]
    assert ops._chunks_with_work(cnt, 6) == []          # the guess was every round: nothing can be left
    assert ops._next_guess(cnt) == 6
