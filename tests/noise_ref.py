"""numpy restatement of the measurement-noise draw of include/fastmpc.h (fmpc_noise): Philox4x32-10 in uint64 arithmetic, the
two 52-bit uniforms, Box-Muller with np.log and np.cos(2*np.pi*u2) / np.sin.  g(seed, step, R, i) is a pure function of its four
arguments; everything is vectorised over R and i."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit values, key: two.  Returns x0..x3 as uint64 arrays holding 32-bit values."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                      # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def uniforms(x):
    """(u1, u2) strictly inside (0, 1) from a Philox block: k + 0.5 with k < 2^52 is exact in a double."""
    s6, s26 = np.uint64(6), np.uint64(26)
    u1 = (((x[0] >> s6) << s26) + (x[1] >> s6)).astype(np.float64) + 0.5
    u2 = (((x[2] >> s6) << s26) + (x[3] >> s6)).astype(np.float64) + 0.5
    return u1 * 2.0 ** -52, u2 * 2.0 ** -52


def normal(seed, step, R, i):
    """g(seed, step, R, i); R and i broadcast against each other."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    R, i = np.broadcast_arrays(np.asarray(R, dtype=np.uint64), np.asarray(i, dtype=np.uint64))
    x = philox4x32_10((i >> np.uint64(1), R, step & 0xFFFFFFFF, step >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    u1, u2 = uniforms(x)
    rho = np.sqrt(-2.0 * np.log(u1))
    return np.where((i & np.uint64(1)) == 0, rho * np.cos(2 * np.pi * u2), rho * np.sin(2 * np.pi * u2))


def fill(batch, p, seed, step=0, first=0, sigma=1.0):
    """(batch, p): sigma_r * g(seed, step, first + r, i)."""
    g = normal(seed, step, first + np.arange(batch)[:, None], np.arange(p)[None, :])
    return np.asarray(sigma, dtype=np.float64).reshape(-1, 1) * g
