"""Float64 restatement of the replica-exchange swap of include/tci.h (tci_dram_run_tempered), for the tests. Host
only: when the swaps run, which pairs they try, the swap ratio with its error bound, the swap's uniform (Philox4x32-10,
Salmon et al. 2011, as the sampler keys it) and what an accepted swap exchanges."""
import numpy as np

TWO_PI = 6.283185307179586
K_LOG = 3       # the device log's error in ulp (1 ulp = 2 u): tci_chainlp's figure
U = 2.0 ** -53
P_SWAP = 6
M32 = 0xFFFFFFFF


def window(adaptint):
    return int(adaptint) if int(adaptint) > 0 else 100


def event_rows(n_steps, adaptint, swap_every):
    """1-based chain rows s = w * win the swap events follow: w % swap_every == 0 and s < n_steps."""
    win, se = window(adaptint), int(swap_every)
    if se <= 0:
        return np.zeros(0, np.int64)
    return np.array([w * win for w in range(1, (int(n_steps) - 1) // win + 1) if w % se == 0], np.int64)


def rungs(ladder):
    """ladder id -> its chains in ascending chain index (the rungs, cold first)."""
    out = {}
    for c, l in enumerate(np.asarray(ladder)):
        if l >= 0:
            out.setdefault(int(l), []).append(c)
    return out


def pairs_tried(ladder, row, adaptint, swap_every):
    """(a, b) chain pairs the event after chain row `row` tries: rungs (r, r + 1) with r = (w / swap_every) mod 2."""
    k = row // window(adaptint) // int(swap_every)
    out = []
    for _, ch in sorted(rungs(ladder).items()):
        out += [(ch[r], ch[r + 1]) for r in range(len(ch) - 1) if r % 2 == k % 2]
    return out


def dev(ss, s2, nobs):
    """tci_chainlp's deviance: a division, a product, a log, a product, a sum."""
    with np.errstate(all="ignore"):
        return np.float64(ss) / np.float64(s2) + np.float64(nobs) * np.log(TWO_PI * np.float64(s2))


def e_dev(ss, s2, nobs):
    """DESIGN.md 7i's bound on the device deviance against the exact one."""
    with np.errstate(all="ignore"):
        L = np.abs(np.log(TWO_PI * s2))
        return 1.01 * U * (np.abs(ss / s2) + nobs * (1.0 + (2 * K_LOG + 1) * L) + np.abs(dev(ss, s2, nobs)))


def logr(beta_a, beta_b, ss_a, s2t_a, ss_b, s2t_b, nobs):
    """(logr, bound): the swap ratio from the stored s2t of both rungs, and how far the device's may lie from it:
    0.5 (beta_a - beta_b) (E_dev_a + E_dev_b) for the two deviances plus 4 u |logr| for the difference, the
    product and the rounding of the two physical sigma2 inside the division."""
    s2a, s2b = np.float64(beta_a) * np.float64(s2t_a), np.float64(beta_b) * np.float64(s2t_b)
    da, db = dev(ss_a, s2a, nobs), dev(ss_b, s2b, nobs)
    lr = (0.5 * (np.float64(beta_a) - np.float64(beta_b))) * (da - db)
    bound = 0.5 * (beta_a - beta_b) * (e_dev(ss_a, s2a, nobs) + e_dev(ss_b, s2b, nobs)) + 4 * U * abs(lr)
    return lr, bound


def philox4x32_10(ctr, key):
    c, k = [int(v) & M32 for v in ctr], [int(v) & M32 for v in key]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
    return c


def uniform_at(seed, key, step, purpose=P_SWAP):
    """The sampler's uniform of stream (seed, key, step, purpose): 53 bits of the first two Philox words, in (0, 1)."""
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step)
    r = philox4x32_10([int(key) & M32, step & M32, ((step >> 32) & 0x00FFFFFF) | (purpose << 24), 0],
                      [seed & M32, seed >> 32])
    return (float(((r[0] << 32) | r[1]) >> 11) + 0.5) * 2.0 ** -53


def accept(lr, u):
    """A logr that is not finite is rejected."""
    return bool(np.isfinite(lr) and u < np.exp(lr))


def exchange(state, a, b, beta, updatesigma):
    """An accepted swap of chains a and b on `state` = dict(theta [n, ld], ss [n], prior [n], s2t [n]), in place:
    theta, ss and prior change places; with updatesigma the physical sigma2 does too."""
    for f in ("theta", "ss", "prior"):
        x = state[f]
        ta = np.array(x[a], copy=True)
        x[a] = x[b]
        x[b] = ta
    if updatesigma:
        s = state["s2t"]
        sa = s[a]
        s[a] = (beta[b] * s[b]) / beta[a]
        s[b] = (beta[a] * sa) / beta[b]
