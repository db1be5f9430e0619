"""Episode metrics of the step engine, with the reference's entry points on top.

The engine keeps, per (env, keyword), three running sums over the days of an episode: profit, the ideal (maximum
expected) profit, and the ideal profit with non-positive days counted as 1.  AKNCP and NCP are functions of those sums
(`akncp_ncp_from_sums`); on several GPUs the per-keyword sums are all-reduced first (`adcraft_amd/distributed.py`).  The
functions named like the reference's (`adcraft/experiment_utils/experiment_metrics.py`) take its [days x keywords]
matrices, form the same sums and go through the same arithmetic, so a notebook that stacks observations day by day gets
the values it got from the reference (pinned by tests/golden/g5_metrics.json).
"""
import numpy as np


# ---------------------------------------------------------------------------------------------- from running sums
def akncp_ncp_from_sums(sum_profit_k, sum_ideal_k, sum_ideal_pos_k=None, count=None):
    """(AKNCP, NCP) from per-keyword sums over the entries (days, or days x envs) of an episode.

    sum_ideal_pos_k: the ideal summed with every non-positive ENTRY replaced by 1 (what the engine accumulates next to
    sum_ideal_k).  When it is not available the replacement is applied to the sums instead, which differs whenever a
    keyword's ideal is non-positive on some days only.
    count: number of entries per keyword; AKNCP is the ratio of two means over them, so it only matters for the last
    bits (the reference divides both by the day count before dividing them by each other).
    """
    profit = np.asarray(sum_profit_k, dtype=np.float64)
    ideal = np.asarray(sum_ideal_k, dtype=np.float64)
    floor_one = np.where(ideal <= 0, 1.0, ideal) if sum_ideal_pos_k is None else np.asarray(sum_ideal_pos_k, dtype=np.float64)
    if count is not None:
        profit, floor_one = profit / count, floor_one / count
    akncp = float(np.median(profit / floor_one))
    whole = ideal.sum()
    ncp = float(np.asarray(sum_profit_k, dtype=np.float64).sum() / (whole if whole > 0.0 else 1.0))
    return akncp, ncp


def _day_sums(kw_profits, ideal_profits):
    """the engine's three per-keyword accumulators, from [days x keywords] matrices"""
    prof = np.asarray(kw_profits, dtype=np.float64)
    ideal = np.asarray(ideal_profits, dtype=np.float64)
    return prof.sum(axis=0), ideal.sum(axis=0), np.where(ideal <= 0, 1.0, ideal).sum(axis=0), prof.shape[0]


def compute_AKNCP(kw_profits, ideal_profits):
    """median over keywords of (mean daily profit) / (mean daily ideal profit, non-positive days counted as 1)
    - the reference's compute_AKNCP on [days x keywords] matrices"""
    s_prof, _, s_floor, days = _day_sums(kw_profits, ideal_profits)
    return np.median((s_prof / days) / (s_floor / days))


def compute_NCP(kw_profits, ideal_profits):
    """total profit over total ideal profit (1 if that is not positive) - the reference's compute_NCP"""
    whole = np.asarray(ideal_profits, dtype=np.float64).sum()
    return np.asarray(kw_profits, dtype=np.float64).sum() / (whole if whole > 0.0 else 1.0)


# ---------------------------------------------------------------------------------------------- ideal profit of a keyword
def expected_profit_curve(vol_mean, bctr, sctr, rev_mean, win_rate_per_bid, price_per_bid):
    """expected daily profit of a keyword at every bid of a grid, never below zero:
    (auctions x win rate x click rate) expected paid clicks, each worth (conversion rate x revenue - price paid).
    The same expression k_ideal_from_curves evaluates per keyword on the device."""
    paid_clicks = vol_mean * np.asarray(win_rate_per_bid, dtype=np.float64) * bctr
    margin = sctr * rev_mean - np.asarray(price_per_bid, dtype=np.float64)
    return np.maximum(paid_clicks * margin, 0.0)


def get_max_expected_bid_profits(kw_params, expected_cpc_per_bid, expected_impression_rate_per_bid):
    """(ideal profit, share of grid bids with positive expected profit, index of the best bid) for a keyword given as
    the reference's parameter tuple ((vol_mean, vol_std), a, b, bctr, sctr, rev_mean, rev_std)"""
    curve = expected_profit_curve(kw_params[0][0], kw_params[3], kw_params[4], kw_params[5],
                                  expected_impression_rate_per_bid, expected_cpc_per_bid)
    best = int(np.argmax(curve))
    return max(0.0, float(curve[best])), np.count_nonzero(curve > 0) / len(curve), best


def bid_curves_from_samples(competitor_bids, bid_array, n_samples=None):
    """win rate and expected price per grid bid from sampled competitor bids (dollars; [1, n] as sample_bids returns them,
    or flat).  n_samples: the divisor of the win rate when it is not the number of samples given.

    A bid wins against the samples it is not below; its win rate is their share.  The expected price is the running
    mean of the sorted samples taken at that count - as the reference has it, one sample further than the winners (the
    cheapest sample the bid loses to is averaged in), capped at the last sample.  adc_bid_curves_from_samples /
    k_ideal_profit compute the same thing from integer cents on the device."""
    ordered = np.sort(np.asarray(competitor_bids, dtype=np.float64)).reshape(-1)
    n = ordered.size if n_samples is None else int(n_samples)
    beaten = np.searchsorted(ordered, bid_array, side="right")
    running_mean = np.cumsum(ordered) / np.arange(1, n + 1)
    return beaten / n, running_mean[np.minimum(beaten, n - 1)]


def get_implicit_kw_bid_cpc_impressions(implicit_keyword, bid_array, n_samples=2048):
    """the reference's estimator: bid curves from n_samples draws of the keyword's competitor bid"""
    return bid_curves_from_samples(implicit_keyword.sample_bids(n_samples), bid_array, n_samples)


def get_explicit_kw_bid_cpc_impressions(explicit_keyword, bid_array, n_samples=2048):
    """the reference's estimator for an ExplicitKeyword (experiment_metrics.py:10-17): the impression rate at every grid bid
    and the median of n_samples sampled costs per click.  StepEngine.bid_curves_build caches the same law for every
    keyword of an engine, with one set of draws shared by the grid's bids."""
    impression_rate = np.array([explicit_keyword.impression_rate(b) for b in bid_array])
    med_cost_per_bid = np.array([np.median(explicit_keyword.cost_per_buyside_click(bid, n_samples)) for bid in bid_array])
    return impression_rate, med_cost_per_bid
