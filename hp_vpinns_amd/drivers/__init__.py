"""Driver scripts.  Shared here: the L-BFGS stage the drivers run after their Adam iterations (`--lbfgs N`)."""
import time


def lbfgs_stage(model, n, error=None, what="relative L2 error", verbose=True, **opts):
    """`n` L-BFGS iterations (`model.train_lbfgs`, options `opts`) after the Adam iterations of a driver; prints the loss and the
    known error `error()` before and after the stage.  Returns train_lbfgs' dict with "seconds", "error_before", "error_after"
    added, or None when n is 0 or None."""
    if not n:
        return None
    l0, e0 = float(model.loss()[0]), (float(error()) if error is not None else float("nan"))
    t0 = time.time()
    info = model.train_lbfgs(int(n), **opts)
    model.h.sync()
    info["seconds"] = time.time() - t0
    l1, e1 = float(model.loss()[0]), (float(error()) if error is not None else float("nan"))
    info["error_before"], info["error_after"] = e0, e1
    if verbose:
        print("L-BFGS stage: %d iterations, %d function evaluations in %.2f s (stopped by %s, %d pairs skipped)"
              % (info["iters"], info["func_evals"], info["seconds"], info["reason"], info["pairs_skipped"]))
        print("  loss %.6e -> %.6e   %s %.4e -> %.4e" % (l0, l1, what, e0, e1))
    return info
