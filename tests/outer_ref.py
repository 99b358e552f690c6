"""NumPy restatement of the outer Reed-Solomon erasure code (gf3_outer_encode / gf3_outer_recover).

Field GF(2^8), polynomial x^8 + x^4 + x^3 + x^2 + 1 (0x11D).  Byte b of a member is its message bits 8b .. 8b+7, most
significant first (np.packbits).  A group has G data and R parity members; parity is systematic from the Cauchy matrix
C[r][j] = 1 / (r xor (R + j)):  P_r[b] = xor_j C[r][j] D_j[b].  Recovery takes the members with iters < 0 as erased,
chooses the first e_d surviving parity rows, inverts A[i][t] = C[r_i][j_t] by Gauss-Jordan and writes
D_erased = A^-1 S,  S_i = P_ri xor xor_{j surviving} C[r_i][j] D_j.  The arithmetic is exact: the GPU is compared with
this file bit for bit."""
import numpy as np

POLY = 0x11D
MAX_R, MAX_N = 16, 255


def _tables():
    exp = np.zeros(510, dtype=np.uint8)
    log = np.zeros(256, dtype=np.int64)
    x = 1
    for i in range(255):
        exp[i] = x
        log[x] = i
        x <<= 1
        if x & 0x100:
            x ^= POLY
    exp[255:] = exp[:255]
    return exp, log


EXP, LOG = _tables()


def mul(a, b):
    """Element-wise product of uint8 arrays (broadcasting)."""
    a, b = np.asarray(a, dtype=np.uint8), np.asarray(b, dtype=np.uint8)
    out = EXP[LOG[a] + LOG[b]]
    return np.where((a == 0) | (b == 0), np.uint8(0), out)


def inv(a):
    a = int(a)
    if a == 0:
        raise ZeroDivisionError("0 has no inverse in GF(256)")
    return int(EXP[255 - LOG[a]])


def check_geometry(G, R, k):
    if not 1 <= R <= MAX_R:
        raise ValueError(f"need 1 <= R <= {MAX_R}")
    if G < 1 or G + R > MAX_N:
        raise ValueError(f"need G >= 1 and G + R <= {MAX_N}")
    if k < 8 or k % 8:
        raise ValueError("k must be a positive multiple of 8")


def cauchy(G, R):
    """uint8 [R, G]: C[r][j] = 1 / (x_r xor y_j), x_r = r, y_j = R + j."""
    return np.array([[inv(r ^ (R + j)) for j in range(G)] for r in range(R)], dtype=np.uint8)


def matvec(M, X):
    """[a, b] coefficients times [b, nbytes] rows -> [a, nbytes]."""
    out = np.zeros((M.shape[0], X.shape[1]), dtype=np.uint8)
    for j in range(M.shape[1]):
        out ^= mul(M[:, j: j + 1], X[j][None, :])
    return out


def invert(A):
    """Gauss-Jordan over GF(256) (a row exchange where a pivot is zero; the result does not depend on it)."""
    e = A.shape[0]
    aug = np.concatenate([A.astype(np.uint8), np.eye(e, dtype=np.uint8)], axis=1)
    for p in range(e):
        piv = p + int(np.flatnonzero(aug[p:, p])[0])
        aug[[p, piv]] = aug[[piv, p]]
        aug[p] = mul(aug[p], np.uint8(inv(aug[p, p])))
        for i in range(e):
            if i != p and aug[i, p]:
                aug[i] ^= mul(aug[i, p], aug[p])
    return aug[:, e:]


def encode(msg_bits, G, R):
    """[NG*G, k] 0/1 message bits, group-major (member j of group g is row g*G + j) -> [NG*R, k] parity bits, row g*R + r."""
    msg_bits = np.asarray(msg_bits, dtype=np.uint8)
    k = msg_bits.shape[1]
    check_geometry(G, R, k)
    NG = msg_bits.shape[0] // G
    D = np.packbits(msg_bits, axis=1).reshape(NG, G, k // 8)
    C = cauchy(G, R)
    P = np.stack([matvec(C, D[g]) for g in range(NG)]) if NG else np.zeros((0, R, k // 8), np.uint8)
    return np.unpackbits(P.reshape(NG * R, k // 8), axis=1)


def recover(bits, iters, G, R):
    """bits [(G+R)*NG, k] in transmitted order (member t of group g is row t*NG + g), iters [(G+R)*NG] (< 0 = erased)
    -> (repaired copy of bits, int32 status [NG])."""
    bits = np.array(bits, dtype=np.uint8)
    iters = np.asarray(iters)
    k = bits.shape[1]
    check_geometry(G, R, k)
    NG = bits.shape[0] // (G + R)
    C = cauchy(G, R)
    status = np.zeros(NG, dtype=np.int32)
    for g in range(NG):
        rows = np.arange(G + R) * NG + g
        erased = iters[rows] < 0
        jd = np.flatnonzero(erased[:G])
        surv_p = np.flatnonzero(~erased[G:])
        e = len(jd)
        if e == 0:
            continue
        if e > len(surv_p):                                     # e_d > R - e_p
            status[g] = -e
            continue
        status[g] = e
        ri = surv_p[:e]                                         # the first e_d surviving parity rows
        js = np.flatnonzero(~erased[:G])
        sym = np.packbits(bits[rows], axis=1)
        S = sym[G + ri] ^ matvec(C[np.ix_(ri, js)], sym[js])
        Dm = matvec(invert(C[np.ix_(ri, jd)]), S)
        bits[rows[jd]] = np.unpackbits(Dm, axis=1)
    return bits, status


# ---- the façade's layout, from the packet count F alone (OFDM.py: outer_layout) --------------------------------------
def capacity(F, per_packet, n):
    """Whole codewords in F packets of per_packet = D*C*mu coded bits."""
    return F * per_packet // n


def groups(F, per_packet, n, G, R):
    return capacity(F, per_packet, n) // (G + R)


def packets_for(n_bits, per_packet, n, k, G, R):
    """The smallest F whose NG(F) groups hold n_bits message bits (at least one group)."""
    F = 1
    while groups(F, per_packet, n, G, R) < 1 or groups(F, per_packet, n, G, R) * G * k < n_bits:
        F += 1
    return F
