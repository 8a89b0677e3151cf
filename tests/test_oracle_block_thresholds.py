"""The oracle's block calling pinned at its exact thresholds, on hand-built layouts (tests/blockcases.py) whose expected
blocks are written out per case from the reference's rules: chain gap -k, minBlockCounts, the canonical match a sub-block
needs, the float32 density test, merge gap -d, -l, the terminal zone and the walk's stop, hasValidOr, the interstitial
fences, minLength and the canonical count of four, the 'b' label, the tips-only regions, the read filter and the GFA
ends' tie.  Each case sits at equality and one step either side; the same cases moved (background in front, filler
matches that put the deciding pair at record 63, 64 or 65 of its list) must give the same blocks, moved."""
import numpy as np
import pytest

from tests import blockcases as BC
from tests import harness as H
from tests.backends import OracleBackend, OracleReadFilter


def oracle(cli):
    return OracleBackend(H.parse_cli(cli))


def as_tuples(blocks):
    return [BC.B(int(b["start"]), int(b["block_len"]), int(b["block_counts"]), int(b["forward_count"]),
                 int(b["canonical_count"]), b["block_label"].decode(), int(b["has_valid_or"])) for b in blocks]


def check_blocks(case, layout, got, shift=0, ctx=""):
    for name, want in (("terminal_blocks", case.term), ("interstitial_blocks", case.its)):
        want = [b.shifted(shift) for b in want]
        assert as_tuples(got[name]) == want, "%s%s %s: oracle %s, expected %s" % (case.name, ctx, name, as_tuples(got[name]), want)
        for b in got[name]:                                 # the fields the tuple leaves out follow from the counts
            assert b["reverse_count"] == b["block_counts"] - b["forward_count"], case.name
            assert b["non_canonical_count"] == b["block_counts"] - b["canonical_count"], case.name


def matches_of(got, full):
    lists = ("all_matches",) if full else ("fwd_matches", "rev_matches")
    out = []
    for name in lists:
        out += [(int(m["position"]), int(m["match_size"]), int(m["is_forward"]), int(m["is_canonical"])) for m in got[name]]
    return sorted(out)


CLIS = sorted({c.command() for c in BC.ALL_CASES} | {"x.fa --fastq-subset " + c[1] for c in BC.READ_CASES})


@pytest.mark.parametrize("cli", CLIS)
def test_background_is_match_free(cli):
    o = oracle(cli.replace("--fastq-subset", "") + " -r -i")
    got = o.scan_segment((BC.BG * 5000).encode(), 0, False)
    assert len(got["all_matches"]) == 0, cli


@pytest.mark.parametrize("case", BC.ALL_CASES, ids=[c.name for c in BC.ALL_CASES])
def test_case_blocks(case):
    o = oracle(case.command())
    got = o.scan_segment(case.layout.seq(), 0, not case.full)
    assert matches_of(got, case.full) == sorted(BC.expected_matches(case)), case.name + ": the layout's match list"
    check_blocks(case, case.layout, got)


@pytest.mark.parametrize("case", BC.ALL_CASES, ids=[c.name for c in BC.ALL_CASES])
def test_case_blocks_at_an_absolute_position(case):
    """abs_pos moves every block start and nothing else"""
    got = oracle(case.command()).scan_segment(case.layout.seq(), 5_000_000_123, not case.full)
    check_blocks(case, case.layout, got, shift=5_000_000_123, ctx=" abs_pos")


MOVABLE = [c for c in BC.ALL_CASES if c.pair]


@pytest.mark.parametrize("case", MOVABLE, ids=[c.name for c in MOVABLE])
def test_moved_cases_keep_their_blocks(case):
    """The placements the device tests use: background in front (the q side keeps its distance to the end), and filler
    matches that put the deciding pair's second record at index 63, 64 and 65 of its list — single copies, each a
    one-match sub-block, so they add no block."""
    spacing = BC.filler_spacing(case.cli, case.full)
    variants = [(case.layout.shifted(4093), 4093)]
    for idx in (63, 64, 65):
        v = BC.at_record_index(case.layout, case.pair, idx, case.side, spacing)
        if v:
            variants.append(v)
    for lay, shift in variants:
        grow = lay.n - case.layout.n
        t = case.t + (grow if case.side in ("p", "q") else 0)
        got = oracle(case.command(t)).scan_segment(lay.seq(), 0, not case.full)
        check_blocks(case, lay, got, shift=shift, ctx=" n=%d shift=%d" % (lay.n, shift))


def test_density_cases_sit_where_float32_puts_them():
    """canCovered >= minBlockDensity * (blockEnd - blockStart) in float32: float32(0.3) * 100 rounds to 30.000002, so 30
    bases of canonical cover over 100 fail where the decimal product (30) would pass; over 99 they pass; -y 0.5 is exact."""
    assert np.float32(np.float32(0.3) * np.float32(100)) > np.float32(30)
    assert not BC.f32_density_side(30, 100, 0.3) and 30 >= 0.3 * 100 - 1e-12        # the decimal product would pass
    assert BC.f32_density_side(30, 99, 0.3)
    assert BC.f32_density_side(6, 12, 0.5) and not BC.f32_density_side(6, 13, 0.5)


def test_first_pattern_of_the_mixed_set_is_the_long_one():
    """getInterstitialBlocks' minLength is 2 * len(patterns.front()): the len cases rely on the 20-base pattern being first"""
    from oracle import pyoracle as po
    assert po.expand_patterns([BC.LONG20, BC.F, BC.R], 0, BC.F)[0][0] == BC.LONG20


@pytest.mark.parametrize("case", BC.READ_CASES, ids=[c[0] for c in BC.READ_CASES])
def test_read_filter_cases(case):
    name, cli, marks, passes = case
    rf = OracleReadFilter(H.parse_cli("--fastq-subset " + cli))
    lay = BC.read_layout(marks)
    assert rf.filter([lay.seq(), lay.mirrored().seq()]) == [passes, passes], name
    for idx in (63, 64, 65):                                 # long lists: the pair at record 63 / 64 / 65, either list
        reads = [BC.long_read(lay, BC.READ_PAIRS[name], idx, cli, BC.F)[0],
                 BC.long_read(lay.mirrored(), _mirror_pair(lay, BC.READ_PAIRS[name]), idx, cli, BC.R)[0]]
        assert rf.filter([r.seq() for r in reads]) == [passes, passes], "%s at record %d" % (name, idx)


def _mirror_pair(lay, pair):
    m = len(lay.marks)
    return (m - 1 - pair[1], m - 1 - pair[0])


@pytest.mark.parametrize("name", sorted(BC.ENDS))
def test_gfa_end_tie_goes_to_the_start_side(name):
    """walkSegment: distToStart <= distToEnd puts a block on the start side (src/input.cpp:849-853)"""
    case = [c for c in BC.ZONE_CASES if c.name == name][0]
    got = oracle(case.command()).scan_segment(case.layout.seq(), 0, True)
    n = case.layout.n
    ends = [0, 0]
    for b in got["terminal_blocks"]:
        rel, ln = int(b["start"]), int(b["block_len"])
        side = 0 if rel <= n - (rel + ln) else 1
        ends[side] = max(ends[side], ln)
    assert tuple(ends) == BC.ENDS[name]


CHAIN_CASES = [c for c in BC.ITS_CASES if c.name.startswith("its_chain_")]


@pytest.mark.parametrize("case", CHAIN_CASES, ids=[c.name for c in CHAIN_CASES])
def test_chain_cases_put_their_gap_where_they_say(case):
    """its_evaluate steps 64 records from the chain's first record: the deciding pair is chain records (62, 63), (63, 64)
    or (64, 65), asserted from the layout (one chain from the first mark up to the pair, every gap within -k)"""
    k = H.parse_cli(case.command()).max_match_dist
    i, j = case.pair
    pos = [p for p, _ in case.layout.marks]
    assert all(b - a <= k for a, b in zip(pos[:i], pos[1:i + 1])), case.name
    assert (i, j) == (int(case.name[-2:]), int(case.name[-2:]) + 1)
    assert pos[j] - pos[i] in (k, k + 1)
