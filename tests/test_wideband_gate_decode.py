"""CPU: what the gate does to the output, with the models and the oracle.  The scene of wideband_gate_check.py - eight channels at
192 ksps, twelve hops, +10 dB pings of standard messages in channels 1, 4 and 6 at different hops, the one in channel 4 across a
hop boundary, channel 2 quiet and always decoded - goes through the float64 channeliser model, wideband.Pings (the default
detector) and wideband.Gate (hold 1, min_up 1), and the oracle decodes the windows (search 0 +- 50 Hz in steps of 2 Hz, depth 6,
threshold 1) with the program's host layer behind it.

The gated run hands the host layer the candidates of the windows in the gate's lists and none for every other window; every
window reaches the SNR tracker either way.  Its lines are exactly the ungated run's lines of the listed (channel, push) pairs, and no
line of a ping channel is lost.  The models alone make this no empty statement: the scene has lines, windows that are not
decoded, and decoded windows without a line (channel 2's, and none of the seed's doing).

CPU simulation on a synthetic scene: nothing here was measured on a GPU.
"""
import wideband_gate_check as gc

CHANNELS, HOPS = 8, 12


def test_the_gated_lines_are_the_ungated_lines_of_the_listed_windows(orc):
    hops, records = gc.scene_model(CHANNELS, HOPS)
    assert len(records) == HOPS - 1
    lists = gc.gate_lists(records)
    assert all(total == len(lst) for lst, total in lists)
    listed = {(int(c), k) for k, (lst, _) in enumerate(lists) for c in lst}
    plain, gated = {}, {}
    for c in range(CHANNELS):
        ow = gc.OracleWindows(hops[c])
        for k, lines in enumerate(ow.lines()):
            plain[(c, k)] = lines
        for k, lines in enumerate(ow.lines({k for (cc, k) in listed if cc == c})):
            gated[(c, k)] = lines
    with_lines = {pair for pair, lines in plain.items() if lines}
    print(f"lists {[[int(c) for c in lst] for lst, _ in lists]}; windows with lines {sorted(with_lines)}")
    # exactly the ungated lines of the listed pairs, and nothing anywhere else
    for pair in plain:
        assert gated[pair] == (plain[pair] if pair in listed else []), pair
    # no line of a ping channel is lost
    for pair in with_lines:
        if pair[0] in gc.SCENE_PING_CHANNELS:
            assert pair in listed and gated[pair] == plain[pair], f"the gate loses the lines of (channel, push) {pair}"
    # every ping channel is decoded somewhere, with its own message
    for c, call in zip(gc.SCENE_PING_CHANNELS, gc.CALLS):
        assert any(f"msg='CQ {call} FN42'" in l for (cc, k), lines in gated.items() if cc == c for l in lines), f"ch={c} never prints {call}"
    # non-vacuity: a decoded line, a window that is not decoded, a decoded window with no line
    assert any(gated[p] for p in listed)
    assert len(listed) < CHANNELS * (HOPS - 1)
    assert any(not plain[p] for p in listed)
    # the ping across the hop boundary keeps the channel in for three pushes
    assert sum(1 for (c, k) in listed if c == gc.SCENE_PING_CHANNELS[1]) >= 3
