#!/usr/bin/env python3
"""Would padding a 17..19-point rule onto the 20x20 tight plan (four channels, three hidden layers) beat the rule's own launches?
pad_probe.py: Poisson-2D / AdvDiff var_form 0 on 16x16 elements, [2,20,20,20,1], the rule as it is (HPV_NO_RULE_PADDING=1) against the
library's advice (hpv_rule_advice: padded onto 20x20 up to five rounds of elements)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hp_vpinns_amd.drivers import advdiff, poisson2d  # noqa: E402
from hp_vpinns_amd.init import xavier_init  # noqa: E402

L = [2, 20, 20, 20, 1]

for prob in ("p2vf0", "advf0"):
    for q in (17, 18, 19):
        nt = q // 2
        for mode in ("rule as it is", "padded onto 20x20"):
            os.environ.pop("HPV_NO_RULE_PADDING", None)
            if mode == "rule as it is":
                os.environ["HPV_NO_RULE_PADDING"] = "1"
            if prob == "p2vf0":
                s = poisson2d.setup(N_el_x=16, N_el_y=16, N_test_x=nt, N_test_y=nt, N_quad=q, with_test_grid=False)
                m = poisson2d.build_model(s, L, var_form=0, init_params=xavier_init(L, 1234))
            else:
                s = advdiff.setup(N_el_x=16, N_el_t=16, N_test_x=nt, N_test_t=nt, N_quad=q, with_test_grid=False)
                m = advdiff.build_model(s, L, var_form=0, init_params=xavier_init(L, 1234, extra=[1.0]))
            m.h.step(64, False)
            t0 = time.perf_counter()
            m.h.step(1000, False)
            print("| %s | %dx%d / %dx%d | %s | %.1f | %s | `%s` |" % (prob, q, q, nt, nt, mode, (time.perf_counter() - t0) / 1000 * 1e6,
                                                                  m.h.pass_structure(), m.h.kernel_variant()), flush=True)
os.environ.pop("HPV_NO_RULE_PADDING", None)
