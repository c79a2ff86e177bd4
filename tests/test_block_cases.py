"""The CPU twin of tests/test_gpu_block_edges.py: what the cases of tests/block_cases.py ARE, stated by stdlib zlib and the C
oracle alone.  Nothing computed by the device enters here.

For every (case, level) the GPU test runs: the oracle's bytes are zlib's, and the pure-Python stream reader agrees with the
oracle's block report.  Then the checklist: every edge of trees.c the GPU test is there for must be reached by at least one
(case, level); the test prints the first one that reaches each item.  A generator that stops reaching its edge (another libz,
another numpy) fails here, on the CPU, and not silently on the device.
"""
import zlib

import numpy as np
import pytest

from oracle import oracle as O
from tests import block_cases as B

CASES = B.cases()
PAIRS = [(name, level) for name in CASES for level in B.LEVELS]

# the pack kernel assembles a block in an image of 8192 words (16 bits for each of a block's 16384 token slots); what a block has
# beyond that goes into the output directly (deflate.hip, section B)
PACK_IMAGE_BITS = 8192 * 32


@pytest.mark.parametrize('name,level', PAIRS)
def test_oracle_bytes_equal_zlib(name, level):
    assert B.oracle_report(name, level)[0] == zlib.compress(CASES[name], level)


@pytest.mark.parametrize('name,level', PAIRS)
def test_stream_reader_agrees_with_the_oracle(name, level):
    """tests/deflate_shape.py read zlib's bytes, the oracle reports what it wrote: same blocks, same places, same sizes."""
    sh, (_, toks, ob) = B.shape(name, level), B.oracle_report(name, level)
    assert len(sh) == len(ob)
    assert sum(o['ntok'] for o in ob) == len(toks)
    for s, o in zip(sh, ob):
        assert (s['btype'], s['last'], s['bit_start']) == (o['btype'], o['last'], o['bit_start'])
        if not s['last']:
            assert s['bit_end'] == o['bit_end']                   # (the oracle's end of a last block is rounded up to a byte)
        else:
            assert (s['bit_end'] + 7) // 8 * 8 == o['bit_end']
        if s['btype'] == 0:
            assert s['len'] == o['in_len']
        else:
            assert s['ntok'] == o['ntok']
        assert s.get('hdr_bits', 0) == o['hdr_bits']
        if s['btype'] == 2:
            assert s['hdr_bits'] + s['body_bits'] == o['opt_len']               # (trees.c counts both, without the 3 type bits)
        if s['btype'] != 2:
            continue
        # an overflow is what makes a code as long as the limit
        assert (o['ovf_l'] > 0) <= (s['l_max_len'] == 15) and (o['ovf_d'] > 0) <= (s['d_max_len'] == 15)
        assert (o['ovf_bl'] > 0) <= (s['bl_max'] == 7)


# ------------------------------------------------------------------------------------------------
# what the single generators are for
# ------------------------------------------------------------------------------------------------
def _dyn(name, level):
    return [(s, o) for s, o in zip(B.shape(name, level), B.oracle_report(name, level)[2]) if s['btype'] == 2]


@pytest.mark.parametrize('level', B.LEVELS)
@pytest.mark.parametrize('seed', [0, 1])
def test_dist_stairs_overflow_the_distance_tree(seed, level):
    for params, ovf in (('1.7_17_13', 2), ('1.66_18_12', 4)):
        s, o = _dyn('dist_stairs_%s_s%d' % (params, seed), level)[-1]
        assert s['last'] and s['d_max_len'] == 15 and o['ovf_d'] == ovf, (params, s['d_max_len'], o['ovf_d'])
        assert s['hdist'] == 30


def _gap_items(R):
    """The run items of R zero lengths (trees.c send_tree)."""
    full, r = divmod(R, 138)
    return [(18, 138)] * full + ([(17, r)] if 3 <= r <= 10 else [(18, r)] if r >= 11 else [])


@pytest.mark.parametrize('level', B.LEVELS)
@pytest.mark.parametrize('R', B.GAP_R)
def test_gap_run_items(R, level):
    """Literals 0 and R + 1 alone: behind the code length of literal 0 come exactly the items of a run of R zeros, then the
    other literal's length and the items of the run up to the end-of-block code (254 - R zeros)."""
    (s, _), = _dyn('gap_%d' % R, level)
    z17_18 = [it for it in s['items'] if it[0] != 16]
    want = _gap_items(R) + _gap_items(254 - R if R < 254 else 0)
    assert z17_18[:len(want)] == want, (R, s['items'])


@pytest.mark.parametrize('level', B.LEVELS)
@pytest.mark.parametrize('n', [600, 3000, 20000])
def test_literal_only_has_no_distance_code(n, level):
    sh = B.shape('literal_only_%d' % n, level)
    assert all(s['btype'] == 2 and s['hlit'] == 257 and s['hdist'] == 2 and s['d_max_len'] == 1 for s in sh), sh
    assert sum(s['ntok'] for s in sh) == n


@pytest.mark.parametrize('level', B.LEVELS)
@pytest.mark.parametrize('ntok', [16382, 16383, 16384])
def test_all_matches_token_counts(ntok, level):
    """Exactly ntok tokens at every level, all but the words' first occurrences matches of length 4; the token buffer fills up
    on a match, and with 16383 tokens the last block is empty."""
    _, toks, ob = B.oracle_report('all_matches_%d' % ntok, level)
    assert len(toks) == ntok
    lit = toks[:, 0] == 0
    assert lit[:640].all() and not lit[640:].any() and (toks[640:, 1] == 1).all()
    assert [o['ntok'] for o in ob] == ([ntok] if ntok < 16383 else [16383, ntok - 16383])
    assert [o['last'] for o in ob] == [0] * (len(ob) - 1) + [1]


def test_fixed_full_block_is_parsed_as_meant():
    """Level 9 parses exactly the tokens the generator meant, and writes them as a fixed block with another block behind it."""
    _, toks, ob = B.oracle_report('fixed_full_block', 9)
    assert [(o['btype'], o['last'], o['ntok']) for o in ob[:3]] == [(0, 0, 16383), (0, 0, 16383), (1, 0, 16383)] and len(ob) == 4
    sh = B.shape('fixed_full_block', 9)[2]
    assert sh['btype'] == 1 and sh['ntok'] == 16383
    t = toks[ob[2]['tok_start']:ob[2]['tok_start'] + 16383]
    lits = t[t[:, 0] == 0, 1]
    assert np.bincount(lits, minlength=256).tolist() == list(B.FIXED_BLOCK_LCOUNTS[:256])
    assert int((t[:, 0] != 0).sum()) == sum(B.FIXED_BLOCK_LCOUNTS[257:]) == sum(B.FIXED_BLOCK_DCOUNTS)
    assert ob[2]['static_len'] - ob[2]['opt_len'] == -79                 # (what the counts were chosen for: ten bytes apart)


def test_skewlen_family_overflows():
    got = set()
    for name in CASES:
        if name.startswith('skewlen'):
            got |= {o['ovf_l'] for o in B.oracle_report(name, 6)[2]} - {0}
    assert len(got) >= 3 and max(got) >= 8, got


# ------------------------------------------------------------------------------------------------
# the checklist
# ------------------------------------------------------------------------------------------------
def _any(pred):
    return lambda sh, ob: any(pred(s, o) for s, o in zip(sh, ob))


def _item(code, rep):
    return _any(lambda s, o: (code, rep) in s.get('items', ()))


def _kind(btype, last):
    return _any(lambda s, o: s['btype'] == btype and s['last'] == last)


def _full_then_empty(sh, ob):
    return len(ob) >= 2 and ob[-2]['ntok'] == 16383 and ob[-1]['ntok'] == 0 and ob[-1]['last'] == 1


CHECKLIST = [
    ('distance overflow >= 2', _any(lambda s, o: o['ovf_d'] >= 2)),
    ('distance overflow >= 4', _any(lambda s, o: o['ovf_d'] >= 4)),
    ('bit-length overflow >= 2', _any(lambda s, o: o['ovf_bl'] >= 2)),
    ('bit-length overflow >= 8', _any(lambda s, o: o['ovf_bl'] >= 8)),
    ('a 15-bit literal/length code', _any(lambda s, o: s.get('l_max_len') == 15)),
    ('a 15-bit distance code', _any(lambda s, o: s.get('d_max_len') == 15)),
    ('a 7-bit bit-length code', _any(lambda s, o: s.get('bl_max') == 7)),
] + [('item (17, %d)' % r, _item(17, r)) for r in range(3, 11)] \
  + [('item (18, %d)' % r, _item(18, r)) for r in (11, 12, 137, 138)] \
  + [('item (16, %d)' % r, _item(16, r)) for r in range(3, 7)] + [
    ('HLIT = 257', _any(lambda s, o: s.get('hlit') == 257)),
    ('HLIT = 286', _any(lambda s, o: s.get('hlit') == 286)),
    ('HDIST = 30', _any(lambda s, o: s.get('hdist') == 30)),
    ('stored block, last', _kind(0, 1)), ('stored block, not last', _kind(0, 0)),
    ('fixed block, last', _kind(1, 1)), ('fixed block, not last', _kind(1, 0)),
    ('dynamic block, last', _kind(2, 1)), ('dynamic block, not last', _kind(2, 0)),
    ('a full block of 16383 tokens, then an empty last block', _full_then_empty),
    ('a header of at least 900 bits', _any(lambda s, o: s.get('hdr_bits', 0) >= 900)),
    ("a block larger than the pack kernel's image", _any(lambda s, o: s['btype'] and s['bit_end'] - s['bit_start'] > PACK_IMAGE_BITS)),
]


def test_checklist(capsys):
    """Every item is reached by at least one (case, level); the items that count over all cases -- at least three distinct
    literal/length overflows with one of 8 or more, every stored-block padding -- are listed with the cases that give the values."""
    first = {}
    ovf_l, pads = {}, {}
    for name, level in PAIRS:
        sh, ob = B.shape(name, level), B.oracle_report(name, level)[2]
        for label, pred in CHECKLIST:
            if label not in first and pred(sh, ob):
                first[label] = (name, level)
        for s, o in zip(sh, ob):
            if o['ovf_l']:
                ovf_l.setdefault(o['ovf_l'], (name, level))
            if s['btype'] == 0:
                pads.setdefault(s['pad'], (name, level))
    lines = ['%-55s %s' % (label, '%s, level %d' % first[label] if label in first else 'NOT REACHED') for label, _ in CHECKLIST]
    lines.append('%-55s %s' % ('literal/length overflow, distinct values', ', '.join('%d (%s, level %d)' % ((v,) + ovf_l[v]) for v in sorted(ovf_l))))
    lines.append('%-55s %s' % ('stored-block padding bits, distinct values', ', '.join('%d (%s, level %d)' % ((v,) + pads[v]) for v in sorted(pads))))
    with capsys.disabled():
        print('\nblock-case checklist (tests/block_cases.py): item, first (case, level) that reaches it')
        print('\n'.join('  ' + ln for ln in lines))
    missing = [label for label, _ in CHECKLIST if label not in first]
    assert not missing, missing
    assert len(ovf_l) >= 3 and max(ovf_l) >= 8, ovf_l
    assert sorted(pads) == list(range(8)), pads            # (the issue asks for three; the cases give every bit phase)


def test_block_report_has_the_overflow_fields():
    """orc_block_info's appended fields where they must be zero: 'abc' is one fixed block -- no tree is 15 high, and there is no
    header.  (Where they are not zero, test_stream_reader_agrees_with_the_oracle holds them to zlib's own bytes.)"""
    _, _, _, ob = O.deflate(b'abc', 6, report=True)
    assert [(o['btype'], o['ovf_l'], o['ovf_d'], o['ovf_bl'], o['hdr_bits']) for o in ob] == [(1, 0, 0, 0, 0)]


# ------------------------------------------------------------------------------------------------
# bytes produced per block (tests/prefix_cases.py places the end of a wanted prefix with them)
# ------------------------------------------------------------------------------------------------
def _nout_streams():
    data = CASES[sorted(CASES)[0]]
    yield 'stored', zlib.compress(data, 0)
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
    yield 'fixed', c.compress(data) + c.flush()
    yield 'empty', zlib.compress(b'', 6)


def test_blocks_report_the_bytes_they_produce():
    """sum(nout) is the length of what zlib inflates: stored-only, Z_FIXED and empty streams, and every (case, level) of the module."""
    from tests.deflate_shape import blocks
    for what, z in _nout_streams():
        sh = blocks(z)
        assert sum(b['nout'] for b in sh) == len(zlib.decompress(z)), what
        assert all(b['nout'] == b['len'] for b in sh if b['btype'] == 0)
        assert {b['btype'] for b in sh} == {{'stored': 0}.get(what, 1)}, what
    for name, level in PAIRS:
        assert sum(b['nout'] for b in B.shape(name, level)) == len(CASES[name]), (name, level)
        assert all(b['nout'] >= b['ntok'] for b in B.shape(name, level) if b['btype'])
