"""The dict FreeWater's device-resident fit returns: `y_corrected` is a key from the start and a value only when it is read."""
import numpy as np


def test_lazy_value_is_made_once_and_only_when_read():
    from amico_amd.models import _LazyResults
    calls = []

    def rows():
        calls.append(1)
        return np.arange(6.0).reshape(2, 3)
    r = _LazyResults({'estimates': np.zeros((2, 2))})
    r.set_lazy('y_corrected', rows)
    assert isinstance(r, dict) and 'y_corrected' in r and list(r) == ['estimates', 'y_corrected'] and len(r) == 2
    assert list(r.keys()) == ['estimates', 'y_corrected'] and r['estimates'].shape == (2, 2)
    assert not calls                                     # membership, keys, iteration, other values: nothing was made
    assert np.array_equal(r['y_corrected'], np.arange(6.0).reshape(2, 3)) and calls == [1]
    assert r['y_corrected'] is r.get('y_corrected') and calls == [1]
    assert [k for k, _ in r.items()] == ['estimates', 'y_corrected'] and len(list(r.values())) == 2 and calls == [1]


def test_lazy_value_through_get_and_assignment():
    from amico_amd.models import _LazyResults
    calls = []
    r = _LazyResults({'a': 0})
    r.set_lazy('c', lambda: calls.append('c') or 3)
    assert r.get('a') == 0 and r.get('missing', 7) == 7 and not calls
    assert r.get('c') == 3 and calls == ['c'] and r.pop('c') == 3 and 'c' not in r
    r.set_lazy('b', lambda: calls.append('b') or 2)
    r['b'] = 20                                          # an assignment replaces the thunk: it never runs
    assert dict(r.items()) == {'a': 0, 'b': 20} and calls == ['c']
    r.set_lazy('d', lambda: 4)
    del r['d']
    assert list(r) == ['a', 'b']


def test_no_copy_or_comparison_sees_the_placeholder():
    """dict(results), {**results}, copy() and == must give the value, not the None that stands in for it"""
    from amico_amd.models import _LazyResults

    def fresh():
        r = _LazyResults({'estimates': 1})
        r.set_lazy('y_corrected', lambda: 5)
        return r
    want = {'estimates': 1, 'y_corrected': 5}
    assert dict(fresh()) == want and {**fresh()} == want and fresh().copy() == want and type(fresh().copy()) is dict
    assert fresh() == want and not (fresh() != want) and want == fresh()
    d = {}
    d.update(fresh())
    assert d == want
