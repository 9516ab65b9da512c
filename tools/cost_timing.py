"""What tools/obstacle_cost.py and tools/episode_obstacle_cost.py share: the
circles, the quantiles and the alternate-and-rotate timing loop."""

RADIUS = 0.02


def circles(n, centre):
    """n small circles (x, y, r), circle i at centre(i): the tool's geometry (the
    test is straight-line code: its cost does not depend on where they are)."""
    return [(*centre(i), RADIUS) for i in range(n)]


def quantile(xs, q):
    xs = sorted(xs)
    pos = q * (len(xs) - 1)
    lo = int(pos)
    hi = min(lo + 1, len(xs) - 1)
    return xs[lo] + (xs[hi] - xs[lo]) * (pos - lo)


def alternate(variants, warmup, rounds, run):
    """run(name, arg, batch, events) for every (name, arg) of `variants`, turn by
    turn in one process: `warmup` untimed rounds (events None), then `rounds`
    timed ones, each call given a fresh device-event pair to record around its
    work; the order rotates, so no variant always follows the same one.  batch
    counts the calls.  Returns {name: [event pairs]} (read them with summary()
    once the device is idle)."""
    import torch
    batch = 0
    for _ in range(warmup):
        for name, arg in variants:
            run(name, arg, batch, None)
            batch += 1
    torch.cuda.synchronize()
    events = {name: [] for name, _ in variants}
    for i in range(rounds):
        k = i % len(variants)
        for name, arg in variants[k:] + variants[:k]:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            run(name, arg, batch, ev)
            batch += 1
            events[name].append(ev)
    return events


def summary(pairs, count_key):
    """One variant's row: the quartiles and the mean of its event pairs, in us."""
    us = [a.elapsed_time(b) * 1e3 for a, b in pairs]
    return {"median_us": quantile(us, 0.5), "p25_us": quantile(us, 0.25),
            "p75_us": quantile(us, 0.75), "mean_us": sum(us) / len(us), count_key: len(us)}
