"""wrap_as_list -- drop-in for rec_now/util/param_normalizer.py (reference rec_now/util/param_normalizer.py:10-24)."""


def wrap_as_list(inputs):
    """inputs itself when it is a list, otherwise [inputs]."""
    if not isinstance(inputs, list):
        inputs = [inputs]
    return inputs
