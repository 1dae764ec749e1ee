"""Local hp-refinement on the host: a mesh of axis-parallel element boxes with per-element test-function counts, and a marking rule
that turns the device-side indicators (hpv_element_indicators) into refinement decisions.  Pure numpy -- nothing here touches a GPU.

Elements need not form a tensor grid: the test functions vanish on every element's boundary, so elements are independent and
hanging nodes are harmless (include/hpvpinn.h, hpv_set_element_boxes).
"""
import numpy as np

# columns of the indicator table (HPV_IND_N of include/hpvpinn.h)
LOSS, ETA2, SUMR2, TOPX, TOPY = range(5)


class ElementMesh:
    """boxes (n, 2*dim) = rows (x0, x1) in 1-D, (x0, x1, y0, y1) in 2-D; nax (n,), nay (n,): active test functions per direction
    (nay is all ones in 1-D).  The element index is the row."""

    def __init__(self, boxes, nax, nay=None):
        self.boxes = np.array(boxes, dtype=np.float64, ndmin=2)
        if self.boxes.shape[1] not in (2, 4):
            raise ValueError("boxes must have 2 (1-D) or 4 (2-D) columns")
        n = self.boxes.shape[0]
        self.nax = np.broadcast_to(np.asarray(nax, dtype=np.int32), (n,)).copy()
        self.nay = np.ones(n, dtype=np.int32) if nay is None else np.broadcast_to(np.asarray(nay, dtype=np.int32), (n,)).copy()
        if self.dim == 1 and np.any(self.nay != 1):
            raise ValueError("a 1-D mesh has no second direction")
        if n < 1 or self.nax.min() < 1 or self.nay.min() < 1:
            raise ValueError("every element needs at least one test function per direction")
        if not np.all(np.isfinite(self.boxes)) or np.any(self.boxes[:, 0::2] >= self.boxes[:, 1::2]):
            raise ValueError("every box needs finite bounds with lower < upper")

    @property
    def dim(self):
        return self.boxes.shape[1] // 2

    def __len__(self):
        return self.boxes.shape[0]

    def copy(self):
        return ElementMesh(self.boxes, self.nax, self.nay)

    @classmethod
    def from_grid(cls, gridx, gridy=None, ntx=1, nty=1):
        """The tensor grid of the constructors as a box list, in the library's order e = ex * ney + ey.  ntx / nty: one count, or
        the per-column / per-row lists `N_testfcn` accepts (element e then gets ntx[ex], nty[ey])."""
        gx = np.asarray(gridx, dtype=np.float64).reshape(-1)
        nex = gx.size - 1
        cx = np.broadcast_to(np.asarray(ntx, dtype=np.int32).reshape(-1), (nex,)) if np.size(ntx) in (1, nex) else None
        if cx is None:
            raise ValueError("ntx needs one entry, or one per element column")
        if gridy is None:
            return cls(np.stack([gx[:-1], gx[1:]], 1), cx)
        gy = np.asarray(gridy, dtype=np.float64).reshape(-1)
        ney = gy.size - 1
        if np.size(nty) not in (1, ney):
            raise ValueError("nty needs one entry, or one per element row")
        cy = np.broadcast_to(np.asarray(nty, dtype=np.int32).reshape(-1), (ney,))
        ex, ey = np.repeat(np.arange(nex), ney), np.tile(np.arange(ney), nex)
        return cls(np.stack([gx[ex], gx[ex + 1], gy[ey], gy[ey + 1]], 1), cx[ex], cy[ey])

    def area(self):
        """total length (1-D) / area (2-D) of the elements"""
        return float(np.prod(self.boxes[:, 1::2] - self.boxes[:, 0::2], axis=1).sum())

    def split(self, e, axis=None):
        """Bisect element e at its midpoint along `axis` (0: x, 1: y / t), or along both (None: four children; in 1-D the same as
        axis 0).  The children REPLACE the parent in place -- rows e, e + 1[, e + 2, e + 3]; every later element moves up -- and
        inherit its counts.  Order: axis 0 -> (left, right); axis 1 -> (lower, upper); None -> (left-lower, left-upper,
        right-lower, right-upper), i.e. the grid order e = ex * 2 + ey of a 2 x 2 grid on the parent.  Returns the number of children."""
        if not 0 <= e < len(self):
            raise IndexError(f"element {e} of {len(self)}")
        if axis not in (0, 1, None) or (axis == 1 and self.dim == 1):
            raise ValueError("axis is 0, 1 (2-D only) or None")
        b = self.boxes[e]
        xs = [(b[0], b[1])]
        ys = [(b[2], b[3])] if self.dim == 2 else [None]
        if axis in (0, None):
            xm = b[0] + (b[1] - b[0]) / 2
            xs = [(b[0], xm), (xm, b[1])]
        if self.dim == 2 and axis in (1, None):
            ym = b[2] + (b[3] - b[2]) / 2
            ys = [(b[2], ym), (ym, b[3])]
        kids = np.array([list(x) + (list(y) if y is not None else []) for x in xs for y in ys])
        k = kids.shape[0]
        self.boxes = np.concatenate([self.boxes[:e], kids, self.boxes[e + 1:]])
        self.nax = np.concatenate([self.nax[:e], np.full(k, self.nax[e]), self.nax[e + 1:]]).astype(np.int32)
        self.nay = np.concatenate([self.nay[:e], np.full(k, self.nay[e]), self.nay[e + 1:]]).astype(np.int32)
        return k

    def raise_p(self, e, axis, p_max):
        """One more test function for element e in direction `axis`, clamped at p_max.  Returns whether the count grew."""
        if axis not in (0, 1) or (axis == 1 and self.dim == 1):
            raise ValueError("axis is 0 or 1 (2-D only)")
        c = self.nax if axis == 0 else self.nay
        if c[e] >= p_max:
            return False
        c[e] += 1
        return True

    def quad_points(self, xi, yi=None, e_begin=0, e_end=None):
        """(n * NQ, dim): the reference nodes mapped into the elements [e_begin, e_end), element-major with q = j * qx + i (x
        fastest) -- the library's layout -- through the library's own expression x0 + (x1 - x0) / 2 * (xi + 1)."""
        b = self.boxes[e_begin:e_end]
        xi = np.asarray(xi, dtype=np.float64).reshape(-1)
        X = b[:, 0:1] + (b[:, 1:2] - b[:, 0:1]) / 2 * (xi[None, :] + 1)                  # (n, qx)
        if self.dim == 1:
            return X.reshape(-1, 1)
        yi = np.asarray(yi, dtype=np.float64).reshape(-1)
        Y = b[:, 2:3] + (b[:, 3:4] - b[:, 2:3]) / 2 * (yi[None, :] + 1)                  # (n, qy)
        n, qx, qy = b.shape[0], xi.size, yi.size
        return np.stack([np.broadcast_to(X[:, None, :], (n, qy, qx)).reshape(-1),
                         np.broadcast_to(Y[:, :, None], (n, qy, qx)).reshape(-1)], 1)

    def jacobians(self):
        """(n,): |J_e| as the library forms it: (x1 - x0) / 2 [* (y1 - y0) / 2]"""
        b = self.boxes
        J = (b[:, 1] - b[:, 0]) / 2
        return J if self.dim == 1 else J * ((b[:, 3] - b[:, 2]) / 2)


def mark(ind, mesh, theta=0.5, smooth=0.1, p_max=None, max_elements=None):
    """A deterministic marking rule: which elements to refine, and how.  Returns a list of (e, action_x, action_y) with each action
    'p' (one more test function in that direction), 'h' (bisect that direction) or None (leave it; always None for y in 1-D),
    sorted by element index.

      * Elements are sorted by eta2 (column 1 of `ind`: the quadrature of the squared strong residual), largest first, ties by
        the lower index.  The shortest prefix whose eta2 sum reaches `theta` (default 0.5) of the total is marked (Doerfler's bulk
        criterion).  Nothing is marked when the total is 0.
      * For a marked element and each direction: when the share of the squared projected residual that sits in the highest active
        test function of that direction, top / sumR2, is below `smooth` (default 0.1) -- the expansion has decayed -- and the count
        is below `p_max`, the action is 'p'; otherwise 'h'.  p_max: one bound or a pair (x, y); default None = the mesh's current
        maximum per direction, i.e. counts only level up to what some element already has.
      * `max_elements` (default None: no bound) is never exceeded: elements are visited in the sorted order, and one whose
        bisections no longer fit keeps only the bisection of its x direction if that fits, else no bisection; its 'p' actions stay.

    The rule is a heuristic: a residual-based indicator with a decay test, nothing more.  No reliability, efficiency or optimality
    of the resulting meshes is claimed."""
    ind = np.asarray(ind, dtype=np.float64)
    n = len(mesh)
    if ind.shape != (n, 5):
        raise ValueError(f"indicator table has shape {ind.shape}, expected {(n, 5)}")
    if p_max is None:
        p_max = (int(mesh.nax.max()), int(mesh.nay.max()))
    px, py = (int(p_max), int(p_max)) if np.isscalar(p_max) else (int(p_max[0]), int(p_max[1]))
    eta = ind[:, ETA2]
    total = float(eta.sum())
    if not total > 0.0:
        return []
    order = sorted(range(n), key=lambda e: (-eta[e], e))
    marked, acc = [], 0.0
    for e in order:
        marked.append(e)
        acc += float(eta[e])
        if acc >= theta * total:
            break
    count = n
    out = []
    for e in marked:
        s = ind[e, SUMR2]
        acts = []
        for axis in range(mesh.dim):
            top, c, cap = ind[e, TOPX + axis], (mesh.nax, mesh.nay)[axis][e], (px, py)[axis]
            acts.append("p" if (s > 0.0 and top / s < smooth and c < cap) else "h")
        if mesh.dim == 1:
            acts.append(None)
        if max_elements is not None:
            grow = {0: 0, 1: 1, 2: 3}[acts.count("h")]
            if count + grow > max_elements:
                if acts[0] == "h" and count + 1 <= max_elements:
                    acts[1] = None if acts[1] == "h" else acts[1]
                else:
                    acts = [None if a == "h" else a for a in acts]
            count += {0: 0, 1: 1, 2: 3}[acts.count("h")]
        if any(a is not None for a in acts):
            out.append((e, acts[0], acts[1]))
    return sorted(out)


def refine(mesh, actions, p_max=None):
    """A new mesh with the actions of `mark` applied (the given mesh is left alone).  Bisections replace the parent in place
    (ElementMesh.split); a 'p' action raises the count of the element, or of all its children when the other direction is bisected."""
    new = mesh.copy()
    if p_max is None:
        p_max = (int(mesh.nax.max()) + 1, int(mesh.nay.max()) + 1)     # (mark has already applied the caller's bound)
    px, py = (int(p_max), int(p_max)) if np.isscalar(p_max) else (int(p_max[0]), int(p_max[1]))
    for e, ax, ay in sorted(actions, reverse=True):                   # from the back: earlier indices stay valid
        k = 1
        if ax == "h" and ay == "h":
            k = new.split(e, None)
        elif ax == "h":
            k = new.split(e, 0)
        elif ay == "h":
            k = new.split(e, 1)
        for c in range(e, e + k):
            if ax == "p":
                new.raise_p(c, 0, px)
            if ay == "p":
                new.raise_p(c, 1, py)
    return new


_FD_STEP = float(np.finfo(np.float64).eps) ** (1.0 / 3.0)      # ~6.1e-6: the step that balances a central difference's two errors
_FD_TOL = 1e4 * _FD_STEP ** 2                                 # ~3.7e-7 per unit of scale, see vpinn._check_ansatz_field

# corners of the reference square in the order of MappedMesh.from_quads, and the bilinear shape functions' signs
_REF_CORNERS = np.array([[-1.0, -1.0], [1.0, -1.0], [1.0, 1.0], [-1.0, 1.0]])


class MappedMesh(ElementMesh):
    """A 2-D mesh of MAPPED elements: each element is a box in a parameter plane (`boxes`, rows (s0, s1, t0, t1)) plus a map into the
    physical plane.  Two kinds:

      * `MappedMesh(boxes, nax, nay, map=phi)`: one global map, `phi(P)` returning `(X (n, 2), A (n, 2, 2))` for parameter points
        P (n, 2) -- the physical points and the Jacobian A[:, a, b] = d x_a / d p_b.  Polar coordinates on (r, theta) boxes are this.
      * `MappedMesh.from_quads(corners, ntx, nty)`: corners (n, 4, 2), counter-clockwise from the image of (-1, -1); every element
        has its own bilinear map of the parameter box [-1, 1]^2 (and of the sub-boxes `split` leaves behind).

    The library never sees the maps: `quad_points` returns the PHYSICAL points, so everything evaluated "at the quadrature points"
    (f, kappa, the ansatz planes) needs no change, and `geometry` returns the Jacobian with respect to each element's REFERENCE
    coordinates, which the model classes fold into the coefficient planes (include/hpvpinn.h, hpv_set_element_points).
    `copy`, `split` and `raise_p` keep the geometry; the children of a split tile their parent exactly.  Checked, each failure a
    ValueError naming the element: finite values and det A > 0 at the corners and the centre of every element (for a bilinear map
    the determinant is bilinear, so the corners decide) and again at every node `geometry` is asked for; for `map=`, the supplied
    Jacobian against central differences of the supplied points there.  2-D only; no triangles."""

    def __init__(self, boxes, nax, nay=None, map=None, corners=None):
        super().__init__(boxes, nax, 1 if nay is None else nay)
        if self.dim != 2:
            raise ValueError("a MappedMesh is 2-D: boxes (n, 4) in the parameter plane")
        if (map is None) == (corners is None):
            raise ValueError("give either map= (one global map) or corners (MappedMesh.from_quads)")
        self.map = map
        self.corners = None if corners is None else np.array(corners, dtype=np.float64).reshape(-1, 4, 2)
        if self.corners is not None and self.corners.shape[0] != len(self):
            raise ValueError("one row of four corners per element")
        self._check()

    @classmethod
    def from_quads(cls, corners, ntx=1, nty=1):
        c = np.array(corners, dtype=np.float64).reshape(-1, 4, 2)
        return cls(np.tile([-1.0, 1.0, -1.0, 1.0], (c.shape[0], 1)), ntx, nty, corners=c)

    def copy(self):
        return MappedMesh(self.boxes, self.nax, self.nay, map=self.map, corners=self.corners)

    def split(self, e, axis=None):
        c = None if self.corners is None else self.corners[e]
        k = super().split(e, axis)                       # (the parameter box is bisected; the map stays)
        if c is not None:
            self.corners = np.concatenate([self.corners[:e], np.repeat(c[None], k, 0), self.corners[e + 1:]])
        return k

    # -- the maps ---------------------------------------------------------------------------------------------------------------
    def _map_points(self, P, elem):
        """physical points (n, 2) and Jacobian d x / d p (n, 2, 2) at parameter points P (n, 2) of the elements `elem` (n,)"""
        if self.map is not None:
            X, A = self.map(P)
            X, A = np.asarray(X, dtype=np.float64), np.asarray(A, dtype=np.float64)
            if X.shape != (P.shape[0], 2) or A.shape != (P.shape[0], 2, 2):
                raise ValueError(f"map(points) returned shapes {X.shape}, {A.shape}; expected {(P.shape[0], 2)}, {(P.shape[0], 2, 2)}")
            return X, A
        c = self.corners[elem]                                               # (n, 4, 2)
        sg, tg = _REF_CORNERS[:, 0][None, :], _REF_CORNERS[:, 1][None, :]    # (1, 4)
        s, t = P[:, 0:1], P[:, 1:2]
        N = (1 + sg * s) * (1 + tg * t) / 4                                  # (n, 4)
        Ns, Nt = sg * (1 + tg * t) / 4, (1 + sg * s) * tg / 4
        X = np.einsum("nc,nca->na", N, c)
        A = np.stack([np.einsum("nc,nca->na", Ns, c), np.einsum("nc,nca->na", Nt, c)], axis=2)
        return X, A

    def _check_points(self, X, A, elem, what):
        bad = ~(np.isfinite(X).all(1) & np.isfinite(A).all((1, 2)))
        if np.any(bad):
            raise ValueError(f"element {int(elem[np.argmax(bad)])}: the map is not finite at {what}")
        det = A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0]
        bad = ~(det > 0.0)
        if np.any(bad):
            i = int(np.argmax(bad))
            raise ValueError(f"element {int(elem[i])}: det of the map's Jacobian is {det[i]:.6g} at {what} (physical point {X[i]}); "
                             "it must be > 0 -- an inverted (clockwise) or non-convex element")

    def _check(self):
        """corners and centre of every parameter box: finite, det > 0, and for map= the Jacobian against central differences"""
        b, n = self.boxes, len(self)
        ref = np.concatenate([_REF_CORNERS, [[0.0, 0.0]]])                   # (5, 2)
        P = np.stack([b[:, None, 0] + (b[:, None, 1] - b[:, None, 0]) / 2 * (ref[None, :, 0] + 1),
                      b[:, None, 2] + (b[:, None, 3] - b[:, None, 2]) / 2 * (ref[None, :, 1] + 1)], axis=2).reshape(-1, 2)
        elem = np.repeat(np.arange(n), ref.shape[0])
        X, A = self._map_points(P, elem)
        self._check_points(X, A, elem, "a corner or the centre")
        if self.map is None:
            return
        for k in range(2):
            e = np.zeros(2)
            e[k] = _FD_STEP
            fd = (self._map_points(P + e, elem)[0] - self._map_points(P - e, elem)[0]) / (2.0 * _FD_STEP)       # d x / d p_k
            scale = np.maximum(1.0, np.maximum(np.abs(X), np.abs(A[:, :, k])))
            bad = (np.abs(fd - A[:, :, k]) > _FD_TOL * scale).any(1)
            if np.any(bad):
                i = int(np.argmax(bad))
                raise ValueError(f"element {int(elem[i])}: the supplied Jacobian column {k} is {A[i, :, k]} at parameter point {P[i]}, "
                                 f"central differences of the supplied points give {fd[i]}")

    # -- what the model classes read ----------------------------------------------------------------------------------------------
    def geometry(self, xi, yi, e_begin=0, e_end=None):
        """(X (n * NQ, 2), A (n * NQ, 2, 2)) of the elements [e_begin, e_end), element-major with q = j * qx + i: the physical
        quadrature points and the Jacobian d x / d (xi, eta) with respect to each element's REFERENCE coordinates (the half widths
        of the parameter box are included).  Finite values and det A > 0 are checked at every node."""
        e_end = len(self) if e_end is None else e_end
        P = ElementMesh.quad_points(self, xi, yi, e_begin, e_end)
        nq = np.size(xi) * np.size(yi)
        elem = np.repeat(np.arange(e_begin, e_end), nq)
        if P.shape[0] == 0:
            return np.zeros((0, 2)), np.zeros((0, 2, 2))
        X, A = self._map_points(P, elem)
        b = self.boxes[elem]
        A = A * np.stack([(b[:, 1] - b[:, 0]) / 2, (b[:, 3] - b[:, 2]) / 2], axis=1)[:, None, :]
        self._check_points(X, A, elem, "a quadrature node")
        return X, A

    def quad_points(self, xi, yi=None, e_begin=0, e_end=None):
        """(n * NQ, 2): the PHYSICAL quadrature points of the elements [e_begin, e_end), in the library's layout"""
        return self.geometry(xi, yi, e_begin, e_end)[0]

    def jacobians(self):
        """(n,): 1 -- the library runs mapped elements as unit elements (the determinant lives in the folded planes)"""
        return np.ones(len(self))

    def area(self, n=8):
        """the physical area: det A integrated by an n x n Gauss-Legendre rule per element -- exact for bilinear and polar maps"""
        x, w = np.polynomial.legendre.leggauss(n)
        A = self.geometry(x, x)[1]
        det = (A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0]).reshape(len(self), n, n)
        return float(np.einsum("ejk,j,k->", det, w, w))
