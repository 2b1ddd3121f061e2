"""The round loop list_stats and adaptive_stats share (PolarCode._stat_rounds) against a plain restatement of the loop each of them
spelled out before: the (t0, T, enabled) it asks its batch function for. No device."""
import numpy as np
import pytest

ERR, RUN = 1, 0          # columns of the fake statistics


def _restated(stats, add_err, max_runs, max_err, batch):
    calls = []
    done, step = 0, int(batch) if batch else max(256, 2 * int(max_err))
    while done < max_runs:
        enabled = ((stats[:, :, ERR] <= max_err) & (stats[:, :, RUN] < max_runs)).astype(np.uint8)
        if not enabled.any():
            break
        T = min(step, max_runs - done)
        calls.append((done, T, enabled.tolist()))
        stats[:, :, RUN] += np.uint64(T) * enabled
        stats[:, :, ERR] += add_err * enabled
        done += T
        if not batch:
            step = min(2 * step, 262144)
    return calls


def _shared(stats, add_err, max_runs, max_err, batch):
    import polar_amd
    calls = []

    def fake(t0, T, enabled):
        assert enabled.dtype == np.uint8 and enabled.shape == stats.shape[:-1]
        calls.append((t0, T, enabled.tolist()))
        stats[..., RUN] += np.uint64(T) * enabled
        stats[..., ERR] += add_err * enabled
    polar_amd.PolarCode._stat_rounds("fake_stats", fake, stats, ERR, RUN, max_runs, max_err, batch)
    return calls


# errors a round adds per cell [2 list sizes, 2 points]: one cell never errs, one passes max_err = 100 in its second round
PATTERN = np.array([[0, 3], [60, 1]], np.uint64)


@pytest.mark.parametrize("batch,max_err,max_runs,add_err,steps", [
    (0, 100, 1000, PATTERN, [256, 512, 232]),                              # 256 first, doubling, the last round cut to max_runs
    (0, 100, 10 ** 6, PATTERN, [256 << i for i in range(10)] + [262144] * 2 + [213824]),      # the cap of 262144
    (7, 100, 20, PATTERN, [7, 7, 6]),
    (0, 100, 1000, np.full((2, 2), 101, np.uint64), [256]),                # every cell over max_err after the first round
])
def test_rounds_equal_the_restated_loop(batch, max_err, max_runs, add_err, steps):
    a, b = np.zeros((2, 2, 2), np.uint64), np.zeros((2, 2, 2), np.uint64)
    want = _restated(a, add_err, max_runs, max_err, batch)
    got = _shared(b, add_err, max_runs, max_err, batch)
    assert got == want
    assert [c[1] for c in got] == steps and [c[0] for c in got] == np.cumsum([0] + steps[:-1]).tolist()
    assert a.tobytes() == b.tobytes()
    if len(steps) > 1 and add_err is PATTERN:
        assert got[0][2] == [[1, 1], [1, 1]] and got[-1][2] == [[1, 1], [0, 1]]          # the cell over max_err left


def test_one_dimensional_cells():
    """adaptive_stats' statistics are [point, column]."""
    stats = np.zeros((3, 2), np.uint64)
    got = _shared(stats, np.array([0, 50, 200], np.uint64), 600, 100, 0)
    assert [(t0, T) for t0, T, _ in got] == [(0, 256), (256, 344)] and [e for _, _, e in got] == [[1, 1, 1], [1, 1, 0]]
