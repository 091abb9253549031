"""CPU: hip_ops.screening_tol is the Python statement of nn1_tol (csrc/exact_distance.h), the relative half-width of the interval
every exact search screens with.  DCI.query_device_k, tools/nnk_bench.py and tests/screening_cases.py take it from there."""
from fractions import Fraction


def test_screening_tol_is_the_closed_form():
    """(dim + 2) u / (1 - (dim + 2) u), u = 2^-24, against exact rational arithmetic.  (dim + 2) u is exact in fp64; the
    subtraction and the division round once each: 2^-52 relative covers both.  At dim = 2^23 - 2 the product is 1/2 and the
    bound is 1, the last dim it says anything for; from (dim + 2) u > 1/2 on it is 1e300 (every pair is measured)."""
    from inclusivegan_amd import hip_ops
    import screening_cases as S
    for dim in (1, 49152, 2 ** 23 - 2):
        x = Fraction(dim + 2, 2 ** 24)
        exact = x / (1 - x)
        got = hip_ops.screening_tol(dim)
        print('dim %d: %.17g, closed form %.17g' % (dim, got, float(exact)))
        assert abs(Fraction(got) - exact) <= exact * Fraction(1, 2 ** 52)
        assert S.nn1_tol(dim) == got
    assert hip_ops.screening_tol(2 ** 23 - 2) == 1.0
    assert hip_ops.screening_tol(2 ** 23) == 1e300
    assert S.nn1_tol(2 ** 23) == 1e300

