"""Numpy reference for the open-set operating points (tests/test_roc_*.py), written from the definitions:

  classes    pair (i, j) is JUNK when ranked_ref.junk_matrix says so and belongs to no class; GENUINE (class 0) = the same pid
             and not junk; IMPOSTOR (class 1) = another pid.
  key        the order-preserving uint32 key of the fp32 distance the matrix holds: bits ^ 0xffffffff when the sign bit is
             set, bits ^ 0x80000000 otherwise.
  operating point for a target rate f:  k = min(floor(float64(f) * float64(N_imp)), N_imp - 1);  tau = the impostor key of
             0-based rank k in ascending order;  a pair is accepted iff key < tau (strict);  FA = #{impostor: key < tau} (<= k
             whatever the ties), TA = #{genuine: key < tau};  far = FA / N_imp, tar = TA / N_gen (nan without genuine pairs);
             threshold = the fp32 value whose key is tau.

roc_ref is the sort-based form (np.sort + searchsorted "left"), hist_ref the np.bincount histograms of one radix pass, and
radix_select the pure-numpy model of the three-pass select the library runs.  The `mutant` switches of roc_ref are the wrong
readings of the definition the tests must be able to tell apart."""
import numpy as np

from ranked_ref import junk_matrix

PASSES = ((0, 11), (11, 11), (22, 10))
RATES = (1e-4, 1e-3, 1e-2, 1e-1, 1.0)


def mono_key(d):
    u = np.ascontiguousarray(d, dtype=np.float32).view(np.uint32)
    return np.where(u >> np.uint32(31), ~u, u ^ np.uint32(0x80000000)).astype(np.uint32)


def key_to_float(key):
    key = np.asarray(key, np.uint32)
    return np.where(key >> np.uint32(31), key ^ np.uint32(0x80000000), ~key).astype(np.uint32).view(np.float32)


def class_keys(dist, q_pids, q_cams, g_pids, g_cams, camsets=False, junk_as_genuine=False):
    """(genuine keys, impostor keys), each a flat uint32 array, of a given fp32 matrix."""
    dist = np.asarray(dist)
    assert dist.dtype == np.float32 and dist.ndim == 2
    junk = junk_matrix(q_pids, q_cams, g_pids, g_cams, camsets)
    same = np.asarray(g_pids, np.int64)[None, :] == np.asarray(q_pids, np.int64)[:, None]
    keys = mono_key(dist)
    gen = same if junk_as_genuine else same & ~junk
    return keys[gen], keys[~same]


def rank_of(rate, n_imp, ceil=False):
    prod = np.float64(rate) * np.float64(n_imp)
    return int(min(np.ceil(prod) if ceil else np.floor(prod), n_imp - 1))


def operating_points(gen, imp, rates, mutant=None):
    """The definition on the two key arrays.  mutant: None, "le" (accept key <= tau), "ceil" (ceil for floor in k)."""
    imp_s, gen_s = np.sort(imp), np.sort(gen)
    n_imp, n_gen = len(imp_s), len(gen_s)
    assert n_imp > 0
    side = "right" if mutant == "le" else "left"
    out = dict(target=np.asarray(rates, np.float64), threshold=[], false_accepts=[], true_accepts=[], k=[])
    for f in rates:
        k = rank_of(f, n_imp, ceil=mutant == "ceil")
        tau = imp_s[k]
        out["k"].append(k)
        out["threshold"].append(tau)
        out["false_accepts"].append(int(np.searchsorted(imp_s, tau, side)))
        out["true_accepts"].append(int(np.searchsorted(gen_s, tau, side)))
    out["k"] = np.asarray(out["k"], np.int64)
    out["key"] = np.asarray(out["threshold"], np.uint32)
    out["threshold"] = key_to_float(out["key"])
    out["false_accepts"] = np.asarray(out["false_accepts"], np.int64)
    out["true_accepts"] = np.asarray(out["true_accepts"], np.int64)
    out["n_impostor"] = np.full(len(rates), n_imp, np.int64)
    out["n_genuine"] = np.full(len(rates), n_gen, np.int64)
    out["far"] = out["false_accepts"] / np.float64(n_imp)
    out["tar"] = out["true_accepts"] / np.float64(n_gen) if n_gen else np.full(len(rates), np.nan)
    return out


def roc_ref(dist, q_pids, q_cams, g_pids, g_cams, rates=RATES, camsets=False, mutant=None):
    """The operating points of a given fp32 matrix, plus hist int64 [2, 2048] / edges fp32 [2048] of the first pass.
    mutant "junk": junk pairs counted as genuine."""
    gen, imp = class_keys(dist, q_pids, q_cams, g_pids, g_cams, camsets, junk_as_genuine=mutant == "junk")
    out = operating_points(gen, imp, rates, mutant)
    out["hist"] = np.stack([np.bincount(gen >> np.uint32(21), minlength=2048), np.bincount(imp >> np.uint32(21), minlength=2048)]).astype(np.int64)
    out["edges"] = key_to_float(np.arange(2048, dtype=np.uint32) << np.uint32(21))
    return out


def hist_of_keys(gen, imp, prefix, prefix_bits, bits):
    """int64 [nsel, 2, 2^bits]: per selector the keys whose leading prefix_bits equal prefix[s], by their next `bits` bits."""
    nsel = len(prefix) if prefix_bits else 1
    out = np.zeros((nsel, 2, 1 << bits), np.int64)
    for c, keys in enumerate((gen, imp)):
        keys = keys.astype(np.uint64)
        digit = ((keys >> np.uint64(32 - prefix_bits - bits)) & np.uint64((1 << bits) - 1)).astype(np.int64)
        lead = keys >> np.uint64(32 - prefix_bits)
        for s in range(nsel):
            sel = np.ones(len(keys), bool) if prefix_bits == 0 else lead == np.uint64(prefix[s])
            out[s, c] = np.bincount(digit[sel], minlength=1 << bits)
    return out


def hist_ref(dist, q_pids, q_cams, g_pids, g_cams, prefix, prefix_bits, bits, camsets=False):
    gen, imp = class_keys(dist, q_pids, q_cams, g_pids, g_cams, camsets)
    return hist_of_keys(gen, imp, prefix, prefix_bits, bits)


def radix_select(gen, imp, rates, passes=PASSES):
    """The three-pass select on the two key arrays, with histograms only: per target the state the select step keeps (rank
    left inside the prefix, prefix, impostors below, genuines below).  Returns (key, false_accepts, true_accepts, k)."""
    n_imp = len(imp)
    assert n_imp > 0
    keys, fas, tas, ks = [], [], [], []
    for f in rates:
        k = rank_of(f, n_imp)
        left, prefix, fa, ta = k, 0, 0, 0
        for pb, bits in passes:
            h = hist_of_keys(gen, imp, [prefix], pb, bits)[0]
            cum = np.cumsum(h[1])
            d = int(np.searchsorted(cum, left, "right"))               # the first digit whose cumulative count exceeds the rank
            below_i = int(cum[d - 1]) if d else 0
            below_g = int(h[0][:d].sum())
            fa += below_i; ta += below_g; left -= below_i
            prefix = (prefix << bits) | d
        keys.append(prefix); fas.append(fa); tas.append(ta); ks.append(k)
    return np.asarray(keys, np.uint32), np.asarray(fas, np.int64), np.asarray(tas, np.int64), np.asarray(ks, np.int64)


def probe_prefixes(imp, prefix_bits, rng=None):
    """Four selectors of `prefix_bits` bits for the histogram tests: two prefixes impostor keys have (the lowest and the most
    frequent), the first one AGAIN (a duplicate), and one no key has."""
    lead = (imp.astype(np.uint64) >> np.uint64(32 - prefix_bits)).astype(np.int64)
    vals, cnt = np.unique(lead, return_counts=True)
    present = set(vals.tolist())
    absent = next(v for v in range(1 << prefix_bits) if v not in present)
    return np.asarray([vals[0], vals[np.argmax(cnt)], vals[0], absent], np.uint32)


def integer_features(nq, ng, D, seed):
    """Features with integer entries in [-2, 2]: squared distances are small integers, so runs of equal keys are long and a
    threshold falls inside one."""
    rng = np.random.default_rng(seed)
    return rng.integers(-2, 3, (nq, D)).astype(np.float32), rng.integers(-2, 3, (ng, D)).astype(np.float32)


def plant_impostor_copies(q, g, q_pids, g_pids):
    """Every fourth query becomes an exact copy of a gallery row of a DIFFERENT pid (the first such row at or after index
    3 i mod ng), then q and g are normalised to unit rows in float32.  The impostor class then holds squared distances that
    round to negative, zero and positive values."""
    q, g = q.copy(), g.copy()
    ng = len(g)
    for i in range(0, len(q), 4):
        j = next(j % ng for j in range(3 * i, 3 * i + ng) if g_pids[j % ng] != q_pids[i])
        q[i] = g[j]
    q = q / np.sqrt((q.astype(np.float64) ** 2).sum(1, keepdims=True)).astype(np.float32)
    g = g / np.sqrt((g.astype(np.float64) ** 2).sum(1, keepdims=True)).astype(np.float32)
    return q.astype(np.float32), g.astype(np.float32)
