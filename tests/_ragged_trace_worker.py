"""Child process of tests/test_gpu_ragged_routes.py::test_traced_leaves: run number sys.argv[1] of that file's trace_runs() on an
exact-f32 handle, one evaluate and one training step.  The parent sets CTX_TRACE_LAUNCH=1 (option trace_launch: one stderr line per
distinct launch) and reads the launched leaves from stderr; one process per run because the trace keeps one set of seen launches per
process."""
import os
import sys


def main():
    from imitation_from_observation_amd import Translator
    from tests.test_gpu_ragged_routes import case_inputs, trace_runs

    name, case, env = trace_runs()[int(sys.argv[1])]
    H, W, d, F, B = case
    cfg, p, (src, ctx, tgt) = case_inputs(case)
    os.environ.update(env)
    with Translator(H, W, d, F, max_batch=B) as tr:
        assert tr.get_option("trace_launch") == 1
        for k, v in env.items():
            assert tr.get_option(k[4:].lower()) == int(v), (k, v)
        tr.set_params(p)
        tr.evaluate(src, ctx, tgt)
        tr.train_step(src, ctx, tgt, lr=0.0)
    return 0


if __name__ == "__main__":
    sys.exit(main())
