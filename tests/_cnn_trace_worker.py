"""Child process of tests/test_gpu_cnn_ops.py::test_traced_leaves: runs the op cases of family sys.argv[1] (trace_families() of that
file) on exact-f32 handles.  The parent sets CTX_TRACE_LAUNCH=1 (option trace_launch: one stderr line per distinct launch) and the
family's switches, and reads the launched leaves from stderr; one process per family because the trace keeps one set of seen launches
per process."""
import sys


def main():
    from tests import _cnn_ref as cr
    from tests.test_gpu_cnn_ops import trace_families

    env, n, cases = trace_families()[sys.argv[1]]
    for case in cases:
        with cr.Handle(case.bufs, case.ops, case.weights(), n) as h:
            h.run(case.frames(n))
    return 0


if __name__ == "__main__":
    sys.exit(main())
