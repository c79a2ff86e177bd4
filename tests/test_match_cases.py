"""The CPU twin of tests/test_gpu_match_edges.py: what the cases of tests/match_cases.py ARE, stated by stdlib zlib and the C
oracle alone.  Nothing computed by the device enters here.

For every (case, level) the GPU test runs: the traced walk gives the oracle's tables, the tables give the oracle's tokens, the
tokens' bytes are zlib's -- and the case's certificate holds: every count that proves the stream sits on its rule is at least 1.
A builder that stops reaching its edge fails here, on the CPU, and not silently on the device.  The last test shows that the
cases discriminate: a reference whose chain budget or distance limit is off by one is caught.
"""
import zlib

import numpy as np
import pytest

from oracle import oracle as O
from tests import match_cases as M

CASES = M.cases()
PAIRS = M.pairs()


@pytest.mark.parametrize('name,level', PAIRS)
def test_case_is_what_it_claims(name, level):
    c = CASES[name]
    tr = M.trace(name, level)
    tf, tq = O.match_tables(c.data, level)
    assert np.array_equal(tr['t_full'], tf) and np.array_equal(tr['t_quarter'], tq)
    z, toks, _, _ = O.deflate(c.data, level, report=True)
    ptoks, _ = O.parse_tables(c.data, tf, tq, level)
    assert np.array_equal(ptoks, toks)
    assert z == zlib.compress(c.data, level)
    if name.startswith('parse_'):                  # (the Python re-walk the parse certificates come from is the parse)
        mine = [(0, c.data[p]) if ln == 0 else (d, ln - 3) for p, ln, d in M.parse_events(c.data, level, tf, tq)[0]]
        assert mine == [tuple(t) for t in toks.tolist()]
    cert = c.cert(level, tr)
    assert cert and all(v >= 1 for v in cert.values()), {k: v for k, v in cert.items() if v < 1}


@pytest.mark.parametrize('level', (1, 2, 3))
def test_fast_levels(level):
    """deflate_fast inserts the strings of a match only up to max_insert_length: both sides, from the oracle's tokens -- and
    the oracle's bytes are zlib's on every case."""
    c = CASES['cmp_len']
    z, toks, _, _ = O.deflate(c.data, level, report=True)
    cert = c.fast_cert(level, toks)
    assert all(v >= 1 for v in cert.values()), cert
    for name, k in CASES.items():
        assert O.deflate(k.data, level) == zlib.compress(k.data, level), name


def test_chunked_stream_reaches_over_its_cuts():
    """In the uncut stream the matches at a chunk's first positions reach back over the cut and the ones before a cut go on over
    it; each chunk alone has neither."""
    data = M.chunked_stream()
    whole, _ = O.match_tables(data, 6)
    cuts = M.CHUNK_CUTS
    assert len(cuts) - 1 >= 3
    for a, b in zip(cuts[1:-1], cuts[2:]):
        alone, _ = O.match_tables(data[a:b], 6)
        k = min(b - a, 100)
        over = sum(1 for i in range(k) if (int(whole[a + i]) & 0xffff) > i)
        assert over >= min(k, 3) - 2 and all((int(alone[i]) & 0xffff) <= i for i in range(b - a))
    for a, b in zip(cuts[:-2], cuts[1:-1]):
        if b - a >= 5003 + 300:
            p = b - 100
            assert (int(whole[p]) >> 16) > 100 >= (int(O.match_tables(data[a:b], 6)[0][p - a]) >> 16) >= 3


def test_every_docstring_names_its_rule():
    assert all(c.doc and len(c.doc) > 60 for c in CASES.values())
    assert max(len(c.data) for c in CASES.values()) <= 300000


def _caught(name, level, **wrong):
    c = CASES[name]
    tf, tq = O.match_tables(c.data, level)
    tr = O.match_trace(c.data, level, **wrong)
    return not (np.array_equal(tr['t_full'], tf) and np.array_equal(tr['t_quarter'], tq))


@pytest.mark.parametrize('level', M.ALL)
def test_a_reference_off_by_one_is_caught(level):
    """The cases discriminate: a walk with one candidate more or less, or a distance limit one further or nearer, gives other
    tables on `budget` and on `dist_limits` (a wrong reference on the CPU; nothing is perturbed on the device)."""
    assert _caught('budget', level, d_budget=1) and _caught('budget', level, d_budget=-1)
    assert _caught('dist_limits', level, d_limit=1) and _caught('dist_limits', level, d_limit=-1)
    assert not _caught('budget', level) and not _caught('dist_limits', level)
