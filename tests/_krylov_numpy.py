"""numpy restatement of the Krylov step kernels (csrc/rmb_krylov.hip: the fused Gram-Schmidt launches in every form;
csrc/rmb_gmres.hip: vec_lincomb_kernel, vec_norm_kernel) -- TEST infrastructure, shared by tests/test_krylov_host.py and
tests/test_gpu_krylov.py.

The algorithm as the kernels run it, on the fp64 inputs as given (V: rows x n, w0: n):

    h1 = V w0,  w1 = w0 - V^T h1;   h2 = V w1,  w2 = w1 - V^T h2;   col = h1 + h2;
    nrm = |w2|   (four launches)   or   sqrt(|w1|^2 - |h2|^2)   (the low-synchronisation ending);   v = w2 / nrm

gram_schmidt(V, w0, dtype) runs it in np.float64 (dots as sums of per-part partials: per chunk of krylov_layout, or per
body / per tile where a finishing launch takes the first pass's dots) or in EXT (np.longdouble, 64-bit mantissa: the
reference).  u = 2^-53, gamma_k = k u / (1 - k u).

Parity with the reference, by a running componentwise bound (reference()):
    e(h1)  = gamma_n |V||w0|
    e(w1)  = gamma_{rows+1} (|w0| + |V^T||h1|) + |V^T| e(h1)
    e(h2)  = gamma_n |V||w1| + |V| e(w1)
    e(col) = e(h1) + e(h2) + u |col|
    e(w2)  = gamma_{rows+1} (|w1| + |V^T||h2|) + e(w1) + |V^T| e(h2)
  "col": |col_got - col| <= e(col), "w": |w_got - w2| <= e(w2), per component.
Statements that hold for ANY basis, the kernel's own outputs on the left, the reference's |h1|, |h2|, s = |w1|^2 on the right:
  "recon"      |w0 - (V^T col + w_out)| <= gamma_{2 rows + 3} (|w0| + |V^T|(|h1| + |h2|))  per component
  "normalise"  |v_next nrm - w_out| <= 3 u |w_out|  per component
  "norm"       four launches: |nrm - |w_out|| <= gamma_{n+2} |w_out|
  "norm_ls"    low-sync: |nrm^2 - |w_out|^2| <= gamma_{n+rows+3} (s + |h2|^2) + 2 |h2| |e(h2)|_2 + |V V^T - I|_2 |h2|^2
               (what the Pythagoras step can guarantee: |w1 - V^T h2|^2 = s - 2 h2.(V w1) + h2.(V V^T h2) and h2 = V w1 up to e(h2))
  "orth"       for a basis that is orthonormal to rounding: |V_r . v_next| <= (gamma_n |V_r|.|w1| + |V V^T - I|_2 |h2|) / |w_out|
  "z"          the fused block product: _rigid_kernels_numpy.block_fraction on the kernel's own v_next
  "lincomb"    |y - (y0 + V^T coef)| <= gamma_{k+1} (|y0| + |V^T||coef|)  per component
  "vnorm"      |out - |v|| <= gamma_{n+2} |v|
An exact breakdown (nrm = 0 stored) leaves inf / nan in every entry of v_next by design: "normalise" and "orth" have no
statement then, the others keep theirs.

Every check yields a FRACTION of its bound.  The asserted bound is min(MARGIN C, 1): C[key] is the worst fraction the fp64
restatement reaches over the cases below (measured and asserted current by tests/test_krylov_host.py, regenerate with

    python -m pytest tests/test_krylov_host.py -k table -s

), MARGIN = 4 covers the kernels' other summation order (four-row lane partials, butterflies, fma).  C comes from the
reference side only, never from a kernel.  The step entries (one Arnoldi / Lanczos step on a resident configuration) are
held to the same keys: their vectors are the operator's output, which the CPU cannot form, so the host test measures their
shapes (n = 3 N + 6 n_bodies or 3 N, rows = j + 1, per-body / per-tile first-pass partials) on random vectors.

Mutants of the restatement (gram_schmidt(..., mutant=), lincomb(..., skip=)): what the suite could not see before.
  ("drop1", k)  the k-th first-pass partial (chunk, body or tile) is left out
  "no_pass2"    h2 = 0, w2 = w1
  "norm_w1"     the norm taken from w1
  "clamp"       the row clamp of the four-row groups stores the duplicate: rows past the last group's first take its dot
  "skip"        one coefficient skipped where the eight-row unrolled loop hands over to the remainder loop"""
import numpy as np

import _mobility_numpy as mn

LONG_DOUBLE = mn.LONG_DOUBLE
EXT = mn.EXT
MARGIN = mn.MARGIN
U = 2.0 ** -53

# worst fraction of the fp64 restatement per statement (see the module text)
C = {
    "col":        0.141,   # measured 0.1402 at ('ortho', 1, 1, 'b', False)
    "lincomb":    0.248,   # measured 0.2478 at ('lincomb', 1, 4608)
    "norm":       0.143,   # measured 0.1421 at ('pc', 1, 3, 0, 2, 'd', False)
    "norm_ls":    1.0,     # measured 1.0000 at ('ortho', 1, 1, 'b', True): V = (0.6), the Gram term of the bound is an identity there
    "normalise":  0.334,   # measured 0.3331 at ('ortho', 1048577, 3, 'a', False)
    "orth":       0.234,   # measured 0.2336 at ('pc', 1, 3, 0, 1, 'a', False)
    "recon":      0.484,   # measured 0.4833 at ('ortho', 65537, 1, 'a', False)
    "vnorm":      0.0045,  # measured 0.0044 at ('vnorm', 255, False)
    "w":          0.162,   # measured 0.1616 at ('ortho', 255, 1, 'a', False)
}

# worst fraction per (form, key) seen by the GPU tests of this process (the last test of the module prints them)
RESULTS = {}


def record(form, key, fraction):
  RESULTS[(form, key)] = max(RESULTS.get((form, key), 0.0), float(fraction))
  return fraction


def bound(key):
  return min(MARGIN * C[key], 1.0)


def gamma(k):
  k = EXT(k)
  return k * EXT(U) / (EXT(1) - k * EXT(U))


def frac(residual, limit):
  """worst |residual| / limit over the elements; where the limit is exactly 0 the residual must be exactly 0 (inf otherwise,
  as for a residual that is not finite)"""
  r = np.abs(np.asarray(residual, dtype=EXT)).reshape(-1)
  s = np.broadcast_to(np.asarray(limit, dtype=EXT), np.shape(residual)).reshape(-1)
  if r.size == 0:
    return 0.0
  if not np.all(np.isfinite(r)) or not np.all(np.isfinite(s)):
    return float("inf")
  zero = s == 0
  if np.any(r[zero] != 0):
    return float("inf")
  if np.all(zero):
    return 0.0
  return float((r[~zero] / s[~zero]).max())


# ---------------------------------------------------------------------------------------------------------------------
# partitions of the first-pass dots
# ---------------------------------------------------------------------------------------------------------------------
def layout(n):
  """krylov_layout: (chunk, n_chunks)"""
  chunk = 256
  while (n + chunk - 1) // chunk > 256 and chunk < 4096:
    chunk *= 2
  return chunk, (n + chunk - 1) // chunk


def chunk_parts(n):
  chunk, nc = layout(n)
  return [np.arange(c * chunk, min(n, (c + 1) * chunk)) for c in range(nc)]


def body_parts(n_bodies, r1, r2):
  """a body's slices of [n_bodies x r1; n_bodies x r2] (rigid_operator_finish_kernel, lanczos_finish_kernel)"""
  top = n_bodies * r1
  return [np.concatenate([np.arange(b * r1, (b + 1) * r1), np.arange(top + b * r2, top + (b + 1) * r2)]) for b in range(n_bodies)]


def tile_parts(n_blobs):
  """192 entries per tile of 64 blobs (plain_finish_kernel)"""
  return [np.arange(192 * t, min(3 * n_blobs, 192 * (t + 1))) for t in range((n_blobs + 63) // 64)]


def unroll_edge(rows):
  """the first row the remainder loop takes after the eight-row unrolled one (the last unrolled row's neighbour)"""
  r = 8 * (rows // 8)
  return r if r < rows else rows - 8


# ---------------------------------------------------------------------------------------------------------------------
# the algorithm
# ---------------------------------------------------------------------------------------------------------------------
def gram_schmidt(V, w0, dtype=np.float64, low_sync=False, parts1=None, mutant=None):
  """-> dict h1, h2, w1, w (= w2), col (rows), nrm, v, s (= |w1|^2)"""
  V = np.asarray(V, dtype=np.float64).astype(dtype)
  w0 = np.asarray(w0, dtype=np.float64).astype(dtype)
  rows, n = V.shape
  chunks = chunk_parts(n)
  parts1 = chunks if parts1 is None else parts1
  kind = mutant[0] if isinstance(mutant, tuple) else mutant
  exact_parts = dtype is not np.float64 and kind not in ("drop1",)

  def dots(w, parts, drop=None):
    if exact_parts:
      h = V @ w
    else:
      h = np.zeros(rows, dtype=dtype)
      for k, p in enumerate(parts):
        if k != drop:
          h = h + V[:, p] @ w[p]
    if kind == "clamp":
      r0 = 4 * ((rows - 1) // 4)
      h[r0 + 1:] = h[r0]
    return h

  def update(w, h, skip=None):
    if skip is not None:
      h = h.copy()
      h[skip] = 0
    return w - V.T @ h

  with np.errstate(all="ignore"):
    h1 = dots(w0, parts1, drop=mutant[1] if kind == "drop1" else None)
    w1 = update(w0, h1, skip=unroll_edge(rows) if kind == "skip" else None)
    if kind == "no_pass2":
      h2, w2 = np.zeros(rows, dtype=dtype), w1
    else:
      h2 = dots(w1, chunks)
      w2 = update(w1, h2)
    col = h1 + h2
    s = sum((w1[p] @ w1[p] for p in chunks), dtype(0))
    if kind == "norm_w1":
      nrm = np.sqrt(s)
    elif low_sync:
      d = s - h2 @ h2
      nrm = np.sqrt(d) if d > 0 else (dtype(0) if d == d else d)
    else:
      nrm = np.sqrt(sum((w2[p] @ w2[p] for p in chunks), dtype(0)))
    v = w2 / nrm
  return dict(h1=h1, h2=h2, w1=w1, w=w2, col=col, nrm=nrm, v=v, s=s)


def reference(V, w0):
  """the EXT run and every bound of the module text that does not depend on the kernel's outputs"""
  V64 = np.ascontiguousarray(V, dtype=np.float64)
  rows, n = V64.shape
  r = gram_schmidt(V64, w0, EXT)
  Ve = V64.astype(EXT)
  aV = np.abs(Ve)
  a = lambda x: np.abs(x)
  w0e = np.asarray(w0, dtype=np.float64).astype(EXT)
  e_h1 = gamma(n) * (aV @ a(w0e))
  e_w1 = gamma(rows + 1) * (a(w0e) + aV.T @ a(r["h1"])) + aV.T @ e_h1
  e_h2 = gamma(n) * (aV @ a(r["w1"])) + aV @ e_w1
  e_col = e_h1 + e_h2 + EXT(U) * a(r["col"])
  e_w2 = gamma(rows + 1) * (a(r["w1"]) + aV.T @ a(r["h2"])) + e_w1 + aV.T @ e_h2
  G = Ve @ Ve.T - np.eye(rows, dtype=EXT)
  gnorm = EXT(np.linalg.norm(G.astype(np.float64), 2))
  h2n2 = r["h2"] @ r["h2"]
  r.update(V=Ve, w0=w0e, rows=rows, n=n, e_col=e_col, e_w=e_w2, gnorm=gnorm,
           recon=gamma(2 * rows + 3) * (a(w0e) + aV.T @ (a(r["h1"]) + a(r["h2"]))),
           norm_ls=gamma(n + rows + 3) * (r["s"] + h2n2) + 2 * np.sqrt(h2n2) * np.sqrt(e_h2 @ e_h2) + gnorm * h2n2,
           orth=gamma(n) * (aV @ a(r["w1"])) + gnorm * np.sqrt(h2n2))
  return r


def fractions(ref, col, w, v, low_sync, orth):
  """col: rows + 1 doubles (the coefficients, then the norm), w, v: n doubles -- the outputs under test.
  -> (dict key -> fraction of the derived bound, breakdown: the stored norm is 0)"""
  rows, n = ref["rows"], ref["n"]
  e = lambda x: np.asarray(x, dtype=np.float64).astype(EXT)
  c, nrm, w, v = e(col[:rows]), e(col[rows]), e(w), e(v)
  f = {"col": frac(c - ref["col"], ref["e_col"]), "w": frac(w - ref["w"], ref["e_w"]),
       "recon": frac(ref["w0"] - (ref["V"].T @ c + w), ref["recon"])}
  wn = np.sqrt(w @ w)
  if low_sync:
    f["norm_ls"] = frac(nrm * nrm - w @ w, ref["norm_ls"])
  else:
    f["norm"] = frac(nrm - wn, gamma(n + 2) * wn)
  breakdown = bool(nrm == 0)
  if not breakdown:
    f["normalise"] = frac(v * nrm - w, 3 * EXT(U) * np.abs(w))
    if orth:
      f["orth"] = frac(ref["V"] @ v, ref["orth"] / wn)
  return f, breakdown


def model_fractions(V, w0, low_sync, orth, parts1=None, mutant=None, ref=None):
  """the fp64 restatement (or a mutant of it) through the same checks"""
  ref = reference(V, w0) if ref is None else ref
  m = gram_schmidt(V, w0, np.float64, low_sync=low_sync, parts1=parts1, mutant=mutant)
  return fractions(ref, np.concatenate([m["col"], [m["nrm"]]]), m["w"], m["v"], low_sync, orth)


# ---------------------------------------------------------------------------------------------------------------------
# linear combination and norm
# ---------------------------------------------------------------------------------------------------------------------
def lincomb(y0, V, coef, dtype=np.float64, skip=None):
  """y0 + V[:k]^T coef -> (y, scale = |y0| + |V^T||coef|)"""
  V = np.asarray(V, dtype=np.float64).astype(dtype)
  cf = np.asarray(coef, dtype=np.float64).astype(dtype)
  y0 = np.asarray(y0, dtype=np.float64).astype(dtype)
  if skip is not None:
    cf = cf.copy()
    cf[skip] = 0
  return y0 + V.T @ cf, np.abs(y0) + np.abs(V).T @ np.abs(np.asarray(coef, dtype=np.float64).astype(dtype))


def lincomb_fraction(y_got, y0, V, coef):
  y, sc = lincomb(y0, V, coef, EXT)
  return frac(np.asarray(y_got, dtype=np.float64).astype(EXT) - y, gamma(len(coef) + 1) * sc)


def vnorm_fraction(got, v):
  ve = np.asarray(v, dtype=np.float64).astype(EXT)
  nrm = np.sqrt(ve @ ve)
  return frac(EXT(got) - nrm, gamma(ve.size + 2) * nrm)


def vnorm_model(v):
  """vec_norm_kernel's order in fp64: 1024 strided chains, then their sum"""
  v = np.asarray(v, dtype=np.float64)
  pad = np.zeros(-(-v.size // 1024) * 1024)
  pad[:v.size] = v
  return float(np.sqrt((pad.reshape(-1, 1024) ** 2).sum(axis=0).sum()))


# ---------------------------------------------------------------------------------------------------------------------
# the cases (the host test measures C over exactly these; the GPU tests run them)
# ---------------------------------------------------------------------------------------------------------------------
def basis(kind, rows, n, rng, m=None):
  """(m, n) float64 with the basis in the first `rows` rows (m >= rows + 1; the rest zero).
  "a": QR-orthonormal.  "b": designed non-orthonormal, rows (q_r + 0.3 q_{r+1}) normalised (Gram off-diagonal 0.28); where
  n has no room for q_rows (rows >= n): random directions of length 0.6.  "d": the same with 0.01 in place of 0.3 -- the
  basis on which the low-synchronisation norm is pinned: its bound carries |V V^T - I|_2 |h2|^2, which on "b" is as large as
  |h2|^2 itself (Pythagoras does not hold there and the bound says so), on "d" a hundredth of it."""
  m = rows + 1 if m is None else m
  V = np.zeros((m, n))
  if kind == "a":
    assert rows < n
    Q, _ = np.linalg.qr(rng.randn(n, rows))
    V[:rows] = Q.T
  elif rows + 1 <= n:
    Q, _ = np.linalg.qr(rng.randn(n, rows + 1))
    B = Q[:, :rows] + (0.3 if kind == "b" else 0.01) * Q[:, 1:]
    V[:rows] = (B / np.linalg.norm(B, axis=0)).T
  else:
    B = rng.randn(rows, n)
    V[:rows] = 0.6 * B / np.linalg.norm(B, axis=1, keepdims=True)
  return V


# n -> the rows run at it.  65536 = 256 chunks of 256; 65537: the chunk doubles, the last chunk holds one element;
# 1048577: the chunk cap of 4096, 257 chunks -- past the 64-lane stride of the partial sums.  rows: every residue of the
# four-row groups of the dots and of the eight-row groups of the updates, one and two rounds of the sixteen rows the four
# waves take together, the maximum.
ORTHO_SHAPES = ((1, (1,)), (255, (1, 3, 4, 5, 8, 9, 15, 16, 17, 33, 64, 65)), (256, (1, 4, 17, 255)), (257, (3, 9, 65, 256)),
                (513, (8, 15, 33, 256)), (2688, (5, 17, 64, 256)), (65536, (5, 17)), (65537, (1, 5)), (1048577, (3, 5)))
# (n_bodies, r1, r2) of the forms that apply blocks in their last launch; rows run with them
PC_SHAPES = ((1, 3, 0), (7, 36, 6), (3, 63, 6), (3, 66, 6), (5, 96, 6), (4, 126, 6), (300, 36, 0))
PC_ROWS = {(1, 3, 0): (1, 2), (7, 36, 6): (4, 17), (3, 63, 6): (5, 16), (3, 66, 6): (9, 33), (5, 96, 6): (8, 60), (4, 126, 6): (3, 61),
           (300, 36, 0): (1, 15)}
LADDER_N, LADDER_ROWS = 2688, 17
LADDER_DELTAS = (1.0, 1e-4, 1e-8, 1e-12, 1e-14, 1e-16, 0.0)
LINCOMB_K = (1, 7, 8, 9, 16, 255, 256)
LINCOMB_N = (1, 255, 256, 257, 4608)
VNORM_N = (1, 255, 1023, 1024, 1025, 4608, 70001)
# the step entries: (n_b, n_bodies); N = 120 is below the symmetric sweep (three-launch fallback, no fused dots), 132 just above
# it, about 400 the ordinary case; 256 / 257 bodies: the last body count with fused dots and the first without
STEP_SHAPES = ((1, 120), (1, 132), (2, 60), (2, 66), (12, 10), (12, 11), (12, 33), (21, 19), (22, 6), (22, 18), (32, 4), (32, 12),
               (33, 4), (33, 12), (42, 3), (42, 10), (12, 256), (12, 257))
STEP_J = (0, 3, 4, 16, 59)
PLAIN_N = (128, 129, 191, 192, 193, 16384, 16448)


def seed_of(*key):
  return sum((i + 1) * 7919 * int(abs(k)) for i, k in enumerate(key)) % (2 ** 31)


def ortho_case(n, rows, kind):
  """-> (V (rows + 1, n), w0)"""
  rng = np.random.RandomState(seed_of(n, rows, ord(kind)))
  return basis(kind, rows, n, rng), rng.randn(n)


def ortho_cases():
  for n, rows_list in ORTHO_SHAPES:
    for rows in rows_list:
      for kind in ("a", "b", "d"):
        if (kind == "a" and rows >= n) or (kind == "d" and (n not in (255, 513, 2688) or rows == 1)):
          continue
        if n > 1000000 and (rows, kind) not in ((3, "a"), (5, "b")):      # (a million columns in long double: one basis per row count)
          continue
        yield n, rows, kind


def ladder_case(delta):
  """basis (a) and w0 = V^T c + delta u, u a unit vector orthogonal to the basis (to rounding)"""
  rng = np.random.RandomState(77)
  n, rows = LADDER_N, LADDER_ROWS
  Q, _ = np.linalg.qr(rng.randn(n, rows + 1))
  V = np.zeros((rows + 1, n))
  V[:rows] = Q[:, :rows].T
  c = rng.randn(rows)
  return V, V[:rows].T @ c + delta * Q[:, rows]


def lincomb_case(k, n):
  """coefficients that cancel: V^T coef = -y0 up to rounding plus a part a thousand times smaller"""
  rng = np.random.RandomState(seed_of(k, n, 5))
  V = rng.randn(k, n)
  coef = rng.randn(k)
  y0 = -(V.T @ coef) + 1e-3 * rng.randn(n)
  return V, coef, y0


def vnorm_case(n, flat=False):
  """entries from 1e-150 to 1e150: the squares stay inside the range of a double, their sum too (there one or two entries
  carry the norm); flat: standard normals, where every entry counts and a dropped one shows"""
  rng = np.random.RandomState(seed_of(n, 9, int(flat)))
  return rng.randn(n) if flat else rng.randn(n) * 10.0 ** rng.uniform(-150, 150, n)


# ---------------------------------------------------------------------------------------------------------------------
# the exact basis (c): rows are coordinate unit vectors, w0 integer-valued -- every result exact
# ---------------------------------------------------------------------------------------------------------------------
EXACT_SHAPES = ((257, 1), (257, 5), (513, 9), (2688, 17), (65537, 5), (65537, 16), (1048577, 5))


def edge_positions(n):
  """both sides of every chunk edge, the first and the last element"""
  chunk, nc = layout(n)
  pos = [0, n - 1]
  for c in range(1, nc):
    pos += [c * chunk - 1, c * chunk]
  return sorted(set(p for p in pos if 0 <= p < n))


def group_edge_rows(rows):
  """both sides of every four- and eight-row group edge, the first and the last row"""
  r = {0, rows - 1}
  for g in range(4, rows, 4):
    r |= {g - 1, g}
  return sorted(x for x in r if 0 <= x < rows)


def exact_basis(n, rows, last_free=False):
  """-> (V (rows + 1, n), positions p_r of the ones, two coordinates off the basis).  The rows at group edges sit on chunk
  edges, taken alternately from the last and the first.  last_free = False: the last element (the whole last chunk at
  n = 65537 and 1048577) carries a basis row, and the second free coordinate is the largest one left -- the last chunk where
  it holds more than one element, the one before it otherwise; last_free = True: the last element stays off the basis and is
  the second free coordinate: 3 and 4 then stand in the first and in the last chunk.  The first free coordinate always lies in
  the first chunk."""
  edges = [p for p in edge_positions(n) if not (last_free and p == n - 1)]
  taken, pos = set(), [None] * rows
  order = group_edge_rows(rows) + [r for r in range(rows) if r not in group_edge_rows(rows)]
  pick = []
  lo, hi = 0, len(edges) - 1
  while lo <= hi:
    pick.append(edges[hi]); hi -= 1
    if lo <= hi:
      pick.append(edges[lo]); lo += 1
  spare = (p for p in range(1, n - 1) if p not in set(edges))
  for k, r in enumerate(order):
    p = pick[k] if k < len(pick) else next(spare)
    while p in taken:
      p = next(spare)
    pos[r] = p
    taken.add(p)
  first = next(p for p in range(2, n) if p not in taken)
  last = next(p for p in range(n - 1, -1, -1) if p not in taken and p != first)
  V = np.zeros((rows + 1, n))
  V[np.arange(rows), pos] = 1.0
  return V, np.array(pos), (first, last)


def edge_one_hots(n, pos):
  """every position on either side of a chunk edge (and the first and the last element) with the basis row that sits there,
  or None: a one-hot w0 = 7 e_p gives col = 7 e_r, w = 0 and the breakdown on a row, col = 0, w = w0, |w| = 7.0 and
  v_next = e_p off the basis -- the dots' partial of that chunk and row, or the chunk's partial of |w|^2, is the only
  non-zero one"""
  where = {int(p): r for r, p in enumerate(pos)}
  return [(p, where.get(p)) for p in edge_positions(n)]


def exact_vectors(n, rows, pos, free):
  """-> list of (name, w0, col (rows + 1) or None, w_out, in_span).  col[rows] = 5.0 where 3 and 4 stand off the basis."""
  out = []
  tail = np.zeros(n)
  tail[free[0]], tail[free[1]] = 3.0, 4.0
  ints = np.zeros(n)
  ints[pos] = np.where(np.arange(rows) % 2 == 0, 1.0, -1.0) * (np.arange(rows) + 2)
  out.append(("ints", ints + tail, np.concatenate([ints[pos], [5.0]]), tail, False))
  for r in group_edge_rows(rows):
    one = np.zeros(n)
    one[pos[r]] = 7.0
    col = np.zeros(rows + 1)
    col[r], col[rows] = 7.0, 5.0
    out.append(("onehot%d" % r, one + tail, col, tail, False))
  out.append(("span", ints, np.concatenate([ints[pos], [0.0]]), np.zeros(n), True))
  out.append(("zero", np.zeros(n), np.zeros(rows + 1), np.zeros(n), True))
  return out
