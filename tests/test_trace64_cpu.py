"""The tracer's fp64 yardstick (tests/trace64.py) on the CPU: every bound of the judge is reachable by the fp32 oracle alone on
every case of the matrix - and a doctored oracle fails it.

Measured here (width-64 bumpy net of seed 1, 1500 rays of seed 7; the test prints every case): undecidable share at most 1.5 %
(`n_rootfind_steps` 0 on `shell`, eval), 1.3 % with line_search_step 0.8, 0.8 % with the oracle's DEFAULT_TRACER, at most 0.6 %
elsewhere and 0 on `away` and `miss`; up to 36 knife-edge rays at the iteration cap per case (radius 1.5), each held to either of
its outcomes; the fp32 oracle's certificate excess / distance from an fp64 candidate per family: shell 1.1e-6 / 2.4e-6 (excess
3.8e-6 with 16 candidates), inside 2.3e-7 / 1.5e-7, graze 1.1e-5 / 3.8e-6 (the sphere intersection cancels: `under` is small),
away 8e-10 / 2e-10 - at most 0.16 of the candidates' fp32 rounding bound.  39 cases + 2 doctored oracles: 50 s on 16 threads."""
import pytest
import torch

import trace64
from oracle import tracer

CASES = trace64.matrix()


def _as_got(r):
    return r['points'], r['hit'], r['dists']


@pytest.mark.parametrize('case', CASES, ids=[c.id for c in CASES])
def test_fp32_oracle_passes_the_judge(case):
    refs = trace64.References(case)
    trace64.judge(refs, _as_got(refs.r32))


def _fails_somewhere(monkeypatch, name, doctored_fn, cases):
    """the judge must refuse a trace of the oracle with tracer.`name` replaced on at least one of `cases`; the references are
    the honest ones, made before the replacement"""
    refs = [trace64.References(case) for case in cases]
    monkeypatch.setattr(tracer, name, doctored_fn)
    failed = []
    for r in refs:
        got = tracer.trace(trace64.make_net(r.case.net)[2], r.o, r.d, r.om, r.p, r.case.training, r.steps)
        try:
            trace64.judge(r, _as_got(got))
        except AssertionError as e:
            failed.append((r.case.id, str(e)[:160]))
    print('refused on %d of %d cases: %s' % (len(failed), len(cases), failed))
    return failed


def test_judge_refuses_a_bracket_that_is_one_sample_off(monkeypatch):
    """first_crossing off by one sample: the bracket is (ind, ind + 1) and the bisection has no sign change to close in on"""
    honest = tracer.first_crossing
    cases = [c for c in CASES if c.family == 'shell' and c.pset in ('default', 'n37_it3') and not c.training]
    assert _fails_somewhere(monkeypatch, 'first_crossing', lambda vals: (honest(vals) + 1).clamp(max=vals.shape[1] - 1), cases)


def test_judge_refuses_an_argmin_over_99_of_100_candidates(monkeypatch):
    """min-SDF search that never looks at its last candidate.  With 100 candidates one ray in a hundred ends beside its
    minimum, by the 2e-5 or so that two neighbours of 100 random depths differ near a smooth minimum - at the edge of what the
    certificate allows (measured: excess 7.9e-6 against a bound of 1.2e-5 on `shell`, default); with 16 and 37 candidates the
    neighbour is far enough for the judge to refuse."""
    honest = tracer.min_sdf_search

    def short(sdf, o, d, t_min, t_max, steps, cnt):
        return honest(sdf, o, d, t_min, t_max, steps[:-1], cnt)
    cases = [c for c in CASES if c.training and c.pset in ('default', 'n16', 'n37_it3') and c.family in ('shell', 'inside')]
    assert _fails_somewhere(monkeypatch, 'min_sdf_search', short, cases)


def test_fp32_oracle_is_unchanged_by_the_dtype_of_its_rays():
    """the dtype-generic oracle in fp32 draws its min-SDF depths where it did and returns fp32; in fp64 it returns fp64"""
    o, d, om, steps = trace64.rays('shell', 64, 3)
    mc, sd, sdf32, sdf64 = trace64.make_net('physg64-smooth')
    r = tracer.trace(sdf32, o, d, om, trace64.tracer_params('default'), True, steps)
    assert r['dists'].dtype == torch.float32 and r['points'].dtype == torch.float32
    r = tracer.trace(sdf64, o.double(), d.double(), om, trace64.tracer_params('default'), True, steps.double())
    assert r['dists'].dtype == torch.float64 and r['points'].dtype == torch.float64
