"""Regenerates tests/golden/lr_schedule.npz from a checkout of the reference:

    python tests/golden/make_goldens_lr.py /path/to/reference

Numbers only: the arguments of the reference's learning-rate schedule `helper` (gaussian_splatting/utils/general_utils.py, what
GaussianModel.update_learning_rate calls at every mapping iteration) and what it returned for them.  The FunctionDef is taken from
the parsed file (the module itself imports the imaging stack) and called with NumPy as its only global.
  args [n,6] float64: step, lr_init, lr_final, lr_delay_steps, lr_delay_mult, max_steps;  lr [n] float64.
Rows: for each schedule the steps -1, 0, 1, max_steps / 2, max_steps, max_steps + 1; the schedules are the reference's
configuration (position_lr_init 0.00016, position_lr_final 0.0000016, delay_mult 0.01, max_steps 30000) under spatial_lr_scale 1
and 6.5, one with both rates 0 (the switched-off branch), and two with lr_delay_steps > 0 (helper's own default is 0, and
update_learning_rate never passes it, so only a direct call reaches that branch)."""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def reference_helper(ref):
    path = os.path.join(ref, "gaussian_splatting", "utils", "general_utils.py")
    fn = [n for n in ast.parse(open(path).read()).body if isinstance(n, ast.FunctionDef) and n.name == "helper"][0]
    ns = {"np": np}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
    return ns["helper"]


def main(ref):
    helper = reference_helper(ref)
    schedules = [(0.00016 * s, 0.0000016 * s, 0, 0.01, 30000) for s in (1.0, 6.5)]
    schedules += [(0.0, 0.0, 0, 0.01, 30000), (0.00016, 0.0000016, 100, 0.01, 30000), (0.01, 0.0001, 2000, 0.25, 1000)]
    args, lr = [], []
    for lr_init, lr_final, delay_steps, delay_mult, max_steps in schedules:
        for step in (-1, 0, 1, max_steps // 2, max_steps, max_steps + 1):
            args.append((step, lr_init, lr_final, delay_steps, delay_mult, max_steps))
            lr.append(float(helper(step, lr_init=lr_init, lr_final=lr_final, lr_delay_steps=delay_steps, lr_delay_mult=delay_mult,
                                   max_steps=max_steps)))
    np.savez(os.path.join(HERE, "lr_schedule.npz"), args=np.asarray(args, np.float64), lr=np.asarray(lr, np.float64))
    print("lr_schedule.npz: %d rows" % len(lr))


if __name__ == "__main__":
    main(sys.argv[1])
