"""The fixed grid of moment tables behind tests/test_annotate_restatement.py and tests/test_gpu_annotate.py: every case is the
input of sgl_annotate_stats (group_n, sum rows x G, rss), drawn from a seeded generator, with planted effects so that the
moderated t runs from 0 to beyond 40 in both signs.  The grid covers residual degrees of freedom from 1 to 1e6, a prior
estimate on both sides of evar = 0 (finite and infinite df_prior), rows = 1, 2, 15 and 3000, an all-zero row, more than half
the rows zero, an empty group and df = 0."""
import numpy as np


def _case(name, seed, rows, group_n, spread, center=True, scale=False, proportion=0.01, tail="pos", zero_rows=(), effect=40.0):
    """spread: the log-scale standard deviation of the rows' true variances (0: equal variances, which puts evar below 0)."""
    rng = np.random.default_rng(seed)
    group_n = np.asarray(group_n, dtype=np.int64)
    G = group_n.shape[0]
    N = int(group_n.sum())
    df = N - int((group_n > 0).sum())
    true_var = np.exp(spread * rng.normal(size=rows))
    s2 = true_var * rng.chisquare(max(df, 1), size=rows) / max(df, 1)
    rss = s2 * max(df, 0)
    with np.errstate(divide="ignore"):
        se = np.sqrt(true_var)[:, None] / np.sqrt(np.maximum(group_n, 1))[None, :]
    # effects in units of the standard error: a ladder from 0 to `effect` in both signs on the first rows, noise elsewhere
    z = rng.normal(size=(rows, G))
    ladder = np.array([0.0, 0.5, -0.5, 2.0, -2.0, 5.0, -5.0, 10.0, -10.0, 20.0, -20.0, effect, -effect])
    for i, v in enumerate(ladder[:rows]):
        z[i, i % G] = v
    mean = 3.0 + z * se
    sums = np.where(group_n[None, :] > 0, mean * group_n[None, :], 0.0)
    for r in zero_rows:
        sums[r, :] = 0.0
        rss[r] = 0.0
    return dict(name=name, rows=rows, G=G, group_n=group_n, sum=sums, rss=rss, center=center, scale=scale, proportion=proportion, tail=tail)


def stats_cases():
    c = []
    c.append(_case("df 1, two rows", 1, 2, [2, 1], 1.0))
    c.append(_case("df 3, fifteen rows, heteroscedastic (evar > 0)", 2, 15, [2, 2, 2], 1.5))
    c.append(_case("df 30, equal variances (evar < 0, infinite prior)", 3, 15, [11, 11, 11], 0.0, tail="std"))
    c.append(_case("df 1e3, 3000 rows", 4, 3000, [300, 200, 503], 0.7, tail="neg"))
    c.append(_case("df 1e6, 3000 rows, near-equal variances", 5, 3000, [500001, 300000, 200002], 0.002, tail="std"))
    c.append(_case("df 1e6, heteroscedastic", 6, 15, [500001, 500001], 1.0))
    c.append(_case("one row (no prior)", 7, 1, [5, 7, 9], 1.0, tail="std"))
    c.append(_case("an all-zero row", 8, 15, [40, 60], 0.8, zero_rows=(3,)))
    c.append(_case("more than half the rows zero", 9, 15, [40, 60, 20], 0.8, zero_rows=tuple(range(0, 15, 2)) + (1,), tail="std"))
    c.append(_case("an empty group", 10, 15, [50, 0, 70, 1], 1.0, tail="neg"))
    c.append(_case("df 0 (every group a single cell)", 11, 15, [1, 1, 1], 1.0))
    c.append(_case("scaled and centred", 12, 15, [25, 30, 45], 1.0, scale=True, tail="std"))
    c.append(_case("not centred, proportion 0.2", 13, 3000, [20, 30], 1.2, center=False, proportion=0.2))
    c.append(_case("scaled with zero rows", 14, 15, [25, 30], 1.0, scale=True, zero_rows=(0, 5)))
    c.append(_case("df 12, 200 groups", 15, 15, [1] * 188 + [2] * 12, 0.5, tail="std"))
    return c


def write_cases(path, cases):
    tails = {"pos": 0, "neg": 1, "std": 2}
    with open(path, "w") as f:
        for c in cases:
            f.write("%d %d %d %d %.17g %d\n" % (c["rows"], c["G"], int(c["center"]), int(c["scale"]), c["proportion"], tails[c["tail"]]))
            f.write(" ".join(str(int(v)) for v in c["group_n"]) + "\n")
            f.write(" ".join("%.17g" % v for v in np.asarray(c["sum"]).T.reshape(-1)) + "\n")   # column-major, row fastest
            f.write(" ".join("%.17g" % v for v in c["rss"]) + "\n")
