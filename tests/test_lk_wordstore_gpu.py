"""Every row of a flagged likelihood launch is written once, by that launch (needs an MI355X).

The one-segment kernels read a row's flag as the 4-byte word of `active` it lies in (the last partial
word and a misaligned array read the byte), and a wave knows the flags of its word's other rows -- so
which wave stores a rejected row's +Inf is a choice of the prologue (one writer
per word was measured and not kept; today every rejected wave stores its own). Whatever the choice,
what can go wrong is a row nobody writes, a row that keeps an earlier launch's value, a row written
with another row's value, or a store past the batch. So every case fills `out` with a sentinel first
and compares bit for bit with the same library's `active=None` launch on the in-bounds rows and +Inf
elsewhere: all 16 flag patterns of the first two words, words without an in-bounds row, flag bytes of
any non-zero value, batches that end in a partial word, a flag array offset by one byte, and two
launches into one `out`.

One synthetic cell per context: N = 2 and 65 (one row per lane) and N = 129 (two rows per lane).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CONSTRUCT = "P2P-MS2v5-LacZ-PP7v4"
SENTINEL = -123.0
POINTS = (2, 65, 129)
RPL = {2: 1, 65: 1, 129: 2}
BATCHES = (1, 3, 4, 5, 8, 13)
BMAX = max(BATCHES)
GUARD = 4  # entries of `out` past the batch, which no launch may touch (a word is four rows)
# what a caller may put into an in-bounds row's flag byte: any non-zero value, top bit set or not
LIVE = np.array([1, 0x80, 0x7F, 0xFF], np.uint8)


def flags_of(bits, B, shift=0):
    """uint8 flags of B rows from a list of 0/1; non-zero bytes cycle through LIVE."""
    bits = np.asarray(bits[:B], np.uint8)
    return np.where(bits != 0, LIVE[(np.arange(B) + shift) % 4], 0).astype(np.uint8)


def word_bits(p):
    return [(p >> j) & 1 for j in range(4)]


class Ctx:
    def __init__(self, n):
        import torch

        from transcriptioncycleinference_amd import Likelihood, from_lists
        from transcriptioncycleinference_amd.data import draw_x0, synthetic_cells

        def fwd(times, theta):
            nan = [np.full(len(t), np.nan) for t in times]
            with Likelihood(from_lists([(t, a, a) for t, a in zip(times, nan)]), CONSTRUCT, device=0) as L:
                return L.forward(theta, np.arange(len(times), dtype=np.int32), grid="interp")

        self.n = n
        self.cells, _ = synthetic_cells(1, n, 20201028 + n, fwd)
        self.lk = Likelihood(self.cells, CONSTRUCT, device=0)
        assert self.lk.info["rows_per_lane"] == RPL[n]
        rng = np.random.default_rng(n)
        self.dev = torch.device("cuda", 0)
        self.theta_h = np.stack([draw_x0(rng, n) for _ in range(BMAX)])
        self.theta = torch.from_numpy(self.theta_h).to(self.dev)
        self.cid = torch.zeros(BMAX, dtype=torch.int32, device=self.dev)
        # the reference, once per batch size and never changed: the same rows with active=None
        self.ref = {B: self.launch(B, None) for B in BATCHES}
        for B in BATCHES:
            assert np.all(np.isfinite(self.ref[B]))
            assert np.array_equal(self.ref[B], self.ref[BMAX][:B])

    def device_flags(self, flags, misaligned=False):
        import torch

        f = torch.from_numpy(np.ascontiguousarray(flags, np.uint8))
        if not misaligned:
            ac = f.to(self.dev)
            assert ac.data_ptr() % 4 == 0
            return ac
        buf = torch.zeros(len(flags) + 1, dtype=torch.uint8, device=self.dev)
        buf[1:] = f.to(self.dev)
        ac = buf[1:]
        assert ac.data_ptr() % 4 == 1 and ac.is_contiguous()
        return ac

    def launch(self, B, flags, out=None, misaligned=False, sync=True):
        """One launch of rows 0..B-1 into a sentinel-filled `out` (or the one given); returns the B values."""
        import torch

        if out is None:
            out = torch.full((B + GUARD,), SENTINEL, dtype=torch.float64, device=self.dev)
        ac = None if flags is None else self.device_flags(flags, misaligned)
        self.lk.ss_batch_device(self.theta[:B], self.cid[:B], out[:B], ac)
        if not sync:
            return out
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.all(got[B:] == SENTINEL), f"N={self.n} B={B}: wrote past the batch: {got[B:]}"
        return got[:B]

    def check(self, B, flags, what, **kw):
        got = self.launch(B, flags, **kw)
        want = np.where(np.asarray(flags[:B]) != 0, self.ref[B], np.inf)
        assert not np.any(got == SENTINEL), f"N={self.n} {what}: rows never written {np.flatnonzero(got == SENTINEL)}"
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), f"N={self.n} {what}: {got} vs {want}"


@pytest.fixture(scope="module")
def ctxs():
    made = {}

    def get(n):
        if n not in made:
            made[n] = Ctx(n)
        return made[n]

    yield get
    for c in made.values():
        c.lk.close()


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("n", POINTS)
def test_every_pattern_of_the_first_two_words(ctxs, n, B):
    """All 16 patterns of word 0 and of word 1 (each beside two different neighbours), the rows after
    them in-bounds or rejected; B = 1, 3, 5 and 13 end in a partial word (the per-row path)."""
    k = ctxs(n)
    for p in range(16):
        for q, tail in ((15 - p, 1), (p, 0), ((5 * p + 3) % 16, p & 1)):
            bits = word_bits(p) + word_bits(q) + [tail, 1 - tail, tail, tail, 1 - tail]
            k.check(B, flags_of(bits, B, shift=p), f"B={B} words {p:04b} {q:04b} tail {tail}")


@pytest.mark.parametrize("n", POINTS)
def test_word_without_in_bounds_rows_and_all_rejected(ctxs, n):
    k = ctxs(n)
    for B in BATCHES:
        k.check(B, np.zeros(B, np.uint8), f"B={B} all rejected")
        k.check(B, flags_of([1] * B, B), f"B={B} all in bounds")
    k.check(8, flags_of([0, 0, 0, 0, 1, 0, 1, 1], 8), "B=8 word 0 empty")
    k.check(8, flags_of([0, 1, 1, 0, 0, 0, 0, 0], 8), "B=8 word 1 empty")
    k.check(13, flags_of([1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0], 13), "B=13 word 1 empty, word 2 last row only")


@pytest.mark.parametrize("n", POINTS)
def test_misaligned_flags_take_the_byte_path(ctxs, n):
    k = ctxs(n)
    rng = np.random.default_rng(100 + n)
    for B in BATCHES:
        for _ in range(3):
            bits = (rng.random(B) < 0.6).astype(np.uint8)
            k.check(B, flags_of(bits, B), f"B={B} offset by one byte {bits}", misaligned=True)
        k.check(B, np.zeros(B, np.uint8), f"B={B} offset by one byte, all rejected", misaligned=True)


@pytest.mark.parametrize("n", POINTS)
def test_second_launch_wins_everywhere(ctxs, n):
    """Two launches back to back into one `out` with different flags: every row holds the second
    launch's value, so no row relies on what an earlier call left there."""
    import torch

    k = ctxs(n)
    rng = np.random.default_rng(200 + n)
    for B in BATCHES:
        for first, second in ((np.ones(B), np.zeros(B)), (np.zeros(B), np.ones(B)),
                              (rng.random(B) < 0.5, rng.random(B) < 0.5), (np.arange(B) % 2, (np.arange(B) + 1) % 2)):
            f1, f2 = flags_of(first.astype(np.uint8), B), flags_of(second.astype(np.uint8), B, shift=1)
            out = k.launch(B, f1, sync=False)
            out = k.launch(B, f2, out=out, sync=False)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert np.all(got[B:] == SENTINEL)
            want = np.where(f2 != 0, k.ref[B], np.inf)
            assert np.array_equal(got[:B].view(np.uint64), want.view(np.uint64)), f"N={n} B={B}: {got[:B]} vs {want}"


def test_forward_modes_unchanged(ctxs, construct, c_oracle):
    """The forward rows (no flags there) against the C oracle, at the bound of tests/test_parity_gpu.py."""
    for n in POINTS:
        k = ctxs(n)
        t = k.cells.cell(0)[0]
        for mode, grid in ((0, "raw"), (1, "interp")):
            ms2, pp7 = k.lk.forward(k.theta_h[:1], np.zeros(1, np.int32), grid=grid)
            m, p = c_oracle.forward(t, construct, k.theta_h[0], mode=mode)
            with np.errstate(invalid="ignore", divide="ignore"):
                e = max(np.nanmax(np.abs(ms2[0, :n] - m) / np.abs(m)), np.nanmax(np.abs(pp7[0, :n] - p) / np.abs(p)))
            print(f"N={n} forward {grid}: max rel err {e:.2e}")
            assert e <= 1e-12


def test_two_segment_construct_flags():
    """The multi-segment variants (their own prologue): flags against active=None on one context."""
    import torch

    from transcriptioncycleinference_amd import Likelihood, from_lists, long_two_loop_construct
    from transcriptioncycleinference_amd.data import draw_x0, synthetic_times

    rng = np.random.default_rng(5)
    n, B = 65, 13
    y = rng.normal(5, 2, (2, n))
    with Likelihood(from_lists([(synthetic_times(rng, n), y[0], y[1])]), long_two_loop_construct(), device=0) as lk:
        dev = torch.device("cuda", 0)
        theta = torch.from_numpy(np.stack([draw_x0(rng, n) for _ in range(B)])).to(dev)
        cid = torch.zeros(B, dtype=torch.int32, device=dev)

        def run(flags):
            out = torch.full((B + GUARD,), SENTINEL, dtype=torch.float64, device=dev)
            lk.ss_batch_device(theta, cid, out[:B], None if flags is None else torch.from_numpy(flags).to(dev))
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert np.all(got[B:] == SENTINEL)
            return got[:B]

        ref = run(None)
        assert np.all(np.isfinite(ref))
        for bits in ([0] * B, [1, 0, 0, 1, 0, 0, 0, 0, 1, 1, 1, 0, 1], [0, 1] * 6 + [0]):
            flags = flags_of(bits, B)
            want = np.where(flags != 0, ref, np.inf)
            assert np.array_equal(run(flags).view(np.uint64), want.view(np.uint64)), bits
