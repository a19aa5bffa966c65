"""Largest lp / gradient errors of the negative-binomial sweeps (the cases of tests/test_gpu_negbin.py::test_negbin_lpgrad)
as fractions of the 1e-10 bars, per sweep group.  Usage: python tools/negbin_errors.py [OUT.json]; needs a GPU."""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import negbin_ref as R
import test_gpu_negbin as T
from stark_amd import engine
ctx = engine.Context(0)
out = {"what": "largest errors of test_negbin_lpgrad's cases as fractions of the bars (lp: 1e-10 max(|lp|, 1); gradient: "
               "1e-10 max(|g_j|, 1e-3 (max|g| + 1))), per sweep group, with and without the count of 2^31 - 1", "groups": {}}
for name, shapes in (("valu", T.VALU), ("k_sweep16", T.S16), ("k_sweep16w", T.S16W), ("gemm64", T.G64)):
    for big in (True, False):
        wl = wg = 0.0
        for n, d, C in shapes:
            rng, X, y, beta = T.make_data(n, d, big=big)
            k = max(1, n // 3)
            m = engine.Model(ctx, "neg_binomial", [{"x": X[:k], "y": y[:k]}, {"x": X, "y": y}])
            q = T.points(rng, beta, C, d)
            lp, g = m.log_density_grad(1, q)
            m.close()
            olp, og = R.ref_lpgrad(X, y, q)
            for c in range(C):
                o = float(olp[c]); ogc = og[c].astype(np.float64)
                wl = max(wl, abs(lp[c] - o) / max(abs(o), 1.0) / 1e-10)
                bar = 1e-10 * np.maximum(np.abs(ogc), (np.abs(ogc).max() + 1.0) * 1e-3)
                wg = max(wg, float((np.abs(g[c] - ogc) / bar).max()))
        out["groups"][f"{name}{'_int32max' if big else '_twin'}"] = {"lp_frac_of_bar": wl, "grad_frac_of_bar": wg}
out_path = sys.argv[1] if len(sys.argv) > 1 else "negbin_errors.json"
json.dump(out, open(out_path, "w"), indent=1)
print(json.dumps(out))
