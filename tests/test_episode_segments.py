"""sampling.episode_segments on a hand-built replay buffer, no GPU.

Three episodes in 9 chronological rows (one state dimension; x -> y is a row with
states x and next_states y):

  rows 0-2  0 -> 1, 1 -> 2, 2 -> 3 (done)         ends with a done in the middle of the buffer
  rows 3-6  10 -> 11, 11 -> 12, 12 -> 13, 13 -> 14   a time-out: no done, but row 7 starts at 20, not 14
  rows 7-8  20 -> 21, 21 -> 22                       the final, unfinished episode
"""
import torch

from drpo_amd.sampling import episode_segments


def _buffer():
    s = torch.tensor([0., 1., 2., 10., 11., 12., 13., 20., 21.]).reshape(-1, 1)
    s2 = torch.tensor([1., 2., 3., 11., 12., 13., 14., 21., 22.]).reshape(-1, 1)
    done = torch.zeros(9, dtype=torch.bool)
    done[2] = True
    return s, s2, done


def _starts(k):
    out = episode_segments(*_buffer(), k)
    assert out.dtype == torch.int64 and out.dim() == 1
    return out.tolist()


def test_exact_start_lists():
    assert _starts(1) == list(range(9))
    assert _starts(2) == [0, 1, 3, 4, 5, 7]
    assert _starts(3) == [0, 3, 4]
    assert _starts(4) == [3]
    assert _starts(5) == []          # longer than every episode
    assert _starts(10) == []         # longer than the buffer


def test_a_done_breaks_a_segment_even_where_the_states_continue():
    """Row 2 is done and row 3 is made to start where it ended: still two episodes."""
    s, s2, done = _buffer()
    s[3] = 3.0
    assert episode_segments(s, s2, done, 2).tolist() == [0, 1, 3, 4, 5, 7]
    done[2] = False                  # without the done the same rows link up
    assert episode_segments(s, s2, done, 2).tolist() == [0, 1, 2, 3, 4, 5, 7]


def test_the_comparison_is_bitwise():
    s, s2, done = _buffer()
    s2[0] = -0.0
    s[1] = 0.0                       # equal as floats, not as bits
    assert 0 not in episode_segments(s, s2, done, 2).tolist()
    nan = float('nan')
    s2[3], s[4] = nan, nan           # the same NaN bits link
    assert 3 in episode_segments(s, s2, done, 2).tolist()


def test_wider_states_and_uint8_dones():
    s, s2, done = _buffer()
    s, s2 = torch.cat([s, -s], 1), torch.cat([s2, -s2], 1)
    assert episode_segments(s, s2, done.to(torch.uint8), 3).tolist() == [0, 3, 4]
    s2[4, 1] += 1.0                  # one component off: rows 4 and 5 no longer link
    assert episode_segments(s, s2, done, 2).tolist() == [0, 1, 3, 5, 7]
