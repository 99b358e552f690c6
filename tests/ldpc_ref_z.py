"""NumPy restatement of the project's quasi-cyclic LDPC codes for any lifting size Z: tests/ldpc_ref.py with Z as an
argument instead of the module constant 64 (that file stays as the record the Z = 64 kernels were held to; with Z = 64
the functions here give the same bits, tests/test_ldpc_wide_cpu.py).  Expansion of a shift table into H, the
dual-diagonal encoder, and the float32 layered normalised min-sum decoder with the exact schedule, tie rule, zero-sign
rule and stop rule of the HIP decoders (csrc/gf3rx_ldpc.hip), which are required to match it bit for bit.

Conventions
  - a shift table is int16 [mb, nb]; -1 is a zero block, s in [0, Z) the circulant P^s whose row z has its one in
    column (z + s) mod Z.  Block columns 0 .. nb-mb-1 carry the message (systematic part), the last mb the parity.
  - codeword bit j*Z + t is bit t of block column j.  LLR > 0 means bit 0; a bit decision is 1 exactly when its
    LLR is < 0 (so +-0 decide 0).
"""
import numpy as np

from tests.ldpc_ref import ALPHA, dual_diagonal, rows_of  # noqa: F401  (neither depends on Z)


def expand(shifts, Z):
    """Binary H [mb*Z, nb*Z] (uint8)."""
    sh = np.asarray(shifts)
    mb, nb = sh.shape
    H = np.zeros((mb * Z, nb * Z), dtype=np.uint8)
    z = np.arange(Z)
    for i in range(mb):
        for j in range(nb):
            if sh[i, j] >= 0:
                H[i * Z + z, j * Z + (z + sh[i, j]) % Z] = 1
    return H


def encode(shifts, msg, Z):
    """msg uint8 [B, k] -> codewords uint8 [B, n], systematic first: lambda_i = sum_j P^{s_ij} m_j over the message
    blocks, p0 = sum_i lambda_i, p1 = lambda_0 + P^x p0, p_{i+1} = lambda_i + p_i (+ p0 at the middle row)."""
    sh = np.asarray(shifts)
    mb, nb = sh.shape
    kb = nb - mb
    dd = dual_diagonal(sh)
    assert dd is not None, "not a dual-diagonal code"
    x, mid = dd
    msg = np.asarray(msg, dtype=np.uint8) & 1
    B = msg.shape[0]
    m = msg.reshape(B, kb, Z)
    z = np.arange(Z)
    lam = np.zeros((B, mb, Z), dtype=np.uint8)
    for i in range(mb):
        for j in range(kb):
            if sh[i, j] >= 0:
                lam[:, i] ^= m[:, j, (z + sh[i, j]) % Z]
    p = np.zeros((B, mb, Z), dtype=np.uint8)
    p[:, 0] = np.bitwise_xor.reduce(lam, axis=1)
    p[:, 1] = lam[:, 0] ^ p[:, 0, (z + x) % Z]
    for i in range(1, mb - 1):
        p[:, i + 1] = lam[:, i] ^ p[:, i] ^ (p[:, 0] if i == mid else 0)
    return np.concatenate([m, p], axis=1).reshape(B, nb * Z)


def syndrome(shifts, cw, Z):
    """H c^T mod 2 for codewords [B, n] -> [B, mb*Z], by circulant addressing (H itself is never formed)."""
    sh = np.asarray(shifts)
    mb, nb = sh.shape
    c = (np.asarray(cw, dtype=np.uint8) & 1).reshape(-1, nb, Z)
    z = np.arange(Z)
    out = np.zeros((c.shape[0], mb, Z), dtype=np.uint8)
    for i, row in enumerate(rows_of(sh)):
        for j, s in row:
            out[:, i] ^= c[:, j, (z + s) % Z]
    return out.reshape(-1, mb * Z)


def decode(shifts, llr, max_iter, Z):
    """Layered normalised min-sum (alpha = 0.75), float32 throughout.

    Block rows are processed in order; for block row i, check row z runs over the non-zero blocks (j, s) in column
    order:  q_e = APP[j][(z+s) % Z] - R_old_e; min1 / its index (first minimum wins: strict <) / min2 / the sign
    product of the q_e (sign(0) = +); then R_new_e = alpha * (e == idx ? min2 : min1), negated when the product of the
    OTHER q signs is negative, and APP[j][(z+s) % Z] = q_e + R_new_e.  R starts at +0.  After every full iteration the
    syndrome of the decisions (APP < 0) is evaluated; a codeword whose syndrome is zero stops there.

    llr float32 [B, n] -> (bits uint8 [B, k], app float32 [B, n], iters int32 [B]: iterations used, -max_iter when the
    syndrome is still non-zero after max_iter iterations)."""
    sh = np.asarray(shifts)
    mb, nb = sh.shape
    kb = nb - mb
    rows = rows_of(sh)
    llr = np.asarray(llr, dtype=np.float32)
    B = llr.shape[0]
    app = llr.reshape(B, nb, Z).copy()
    R = [np.zeros((B, len(r), Z), dtype=np.float32) for r in rows]
    iters = np.full(B, -max_iter, dtype=np.int32)
    act = np.arange(B)
    z = np.arange(Z)
    for it in range(max_iter):
        if len(act) == 0:
            break
        A = app[act]
        for i, row in enumerate(rows):
            Ri = R[i][act]
            d = len(row)
            q = np.empty((len(act), d, Z), dtype=np.float32)
            for e, (j, s) in enumerate(row):
                q[:, e] = A[:, j, (z + s) % Z] - Ri[:, e]
            aq = np.abs(q)
            m1 = np.full((len(act), Z), np.inf, dtype=np.float32)
            m2 = np.full((len(act), Z), np.inf, dtype=np.float32)
            idx = np.zeros((len(act), Z), dtype=np.int64)
            for e in range(d):
                v = aq[:, e]
                lt1 = v < m1
                lt2 = ~lt1 & (v < m2)
                m2 = np.where(lt1, m1, np.where(lt2, v, m2))
                idx = np.where(lt1, e, idx)
                m1 = np.where(lt1, v, m1)
            neg = q < 0
            par = np.bitwise_xor.reduce(neg, axis=1)
            for e, (j, s) in enumerate(row):
                mag = np.where(idx == e, m2, m1)
                r = ALPHA * mag
                r = np.where(par ^ neg[:, e], -r, r)
                Ri[:, e] = r
                A[:, j, (z + s) % Z] = q[:, e] + r
            R[i][act] = Ri
        app[act] = A
        bad = np.zeros((len(act), Z), dtype=bool)
        hard = A < 0
        for row in rows:
            par = np.zeros((len(act), Z), dtype=bool)
            for j, s in row:
                par ^= hard[:, j, (z + s) % Z]
            bad |= par
        done = ~bad.any(axis=1)
        iters[act[done]] = it + 1
        act = act[~done]
    bits = (app[:, :kb, :] < 0).astype(np.uint8).reshape(B, kb * Z)
    return bits, app.reshape(B, nb * Z), iters


def check_properties(shifts, Z, seed=0, n_msg=8):
    """Every property the generator asserts; returns a list of one-line reports (raises AssertionError otherwise)."""
    sh = np.asarray(shifts)
    mb, nb = sh.shape
    kb = nb - mb
    out = []
    assert sh.dtype == np.int16 and ((sh >= -1) & (sh < Z)).all(), f"shifts must be int16 in [-1, {Z})"
    n4 = 0
    for i in range(mb):
        for i2 in range(i + 1, mb):
            for j in range(nb):
                for j2 in range(j + 1, nb):
                    if min(sh[i, j], sh[i, j2], sh[i2, j], sh[i2, j2]) < 0:
                        continue
                    n4 += 1
                    assert (int(sh[i, j]) - int(sh[i, j2]) + int(sh[i2, j2]) - int(sh[i2, j])) % Z != 0, \
                        f"4-cycle at rows {i},{i2} cols {j},{j2}"
    out.append(f"no 4-cycles mod {Z} ({n4} all-non-zero 2x2 block sub-matrices checked)")
    deg = (sh[:, :kb] >= 0).sum(axis=0)
    assert deg.min() >= 3, f"information column of degree {deg.min()}"
    out.append(f"information column degrees {deg.min()}..{deg.max()} (>= 3)")
    dd = dual_diagonal(sh)
    assert dd is not None, "parity part is not dual-diagonal"
    out.append(f"dual-diagonal parity part: x = {dd[0]}, middle row {dd[1]}")
    rng = np.random.default_rng(seed)
    msg = rng.integers(0, 2, size=(n_msg, kb * Z), dtype=np.uint8)
    cw = encode(sh, msg, Z)
    assert not syndrome(sh, cw, Z).any(), "H c^T != 0"
    assert np.array_equal(cw[:, :kb * Z], msg), "encoder is not systematic"
    out.append(f"H c^T = 0 for {n_msg} random messages")
    return out
