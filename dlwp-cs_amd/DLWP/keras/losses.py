"""
The two keras losses the DLWP scripts use, as `tensorflow.keras.losses` defines them: the mean over the LAST axis; keras'
loss reduction then averages the returned tensor over everything else.  They run on host arrays (numpy or torch), for tests
and for users; `Model.compile` recognises them by identity and runs its HIP kernels in their place (DLWP.ops.loss_stats).
"""
import collections


def _mean_last(x):
    if hasattr(x, 'detach'):                # torch
        return x.mean(dim=-1)
    import numpy as np
    return np.mean(x, axis=-1)


def _abs(x):
    if hasattr(x, 'detach'):
        return x.abs()
    import numpy as np
    return np.abs(x)


def mean_squared_error(y_true, y_pred):
    return _mean_last((y_pred - y_true) ** 2)


def mean_absolute_error(y_true, y_pred):
    return _mean_last(_abs(y_pred - y_true))


mse = MSE = mean_squared_error
mae = MAE = mean_absolute_error

_BY_NAME = {'mean_squared_error': mean_squared_error, 'mse': mean_squared_error, 'MSE': mean_squared_error,
            'mean_absolute_error': mean_absolute_error, 'mae': mean_absolute_error, 'MAE': mean_absolute_error}


def get(identifier):
    """keras.losses.get: None -> None, a name -> the function, a callable -> itself."""
    if identifier is None:
        return None
    if isinstance(identifier, str):
        fn = _BY_NAME.get(identifier)
        if fn is None:
            raise ValueError('Unknown loss function: %s' % identifier)
        return fn
    if callable(identifier):
        return identifier
    raise ValueError('Could not interpret loss function identifier: %r' % (identifier,))


# ---- what the engine runs for a loss (DLWP.keras.Model.compile) ---------------------------------------------------------
# kind 'mse' / 'mae' / 'acc'; weights: the latitude weight field of DLWP.custom.latitude_weighted_loss (or None); clim: the
# climatology of DLWP.custom.anomaly_correlation_loss, shape (1, ...) (or None); regularize / reverse: the anomaly-correlation options;
# masked: None, or the normalisation of DLWP.custom.masked_loss ('all' / 'valid': NaN targets are holes)
LossSpec = collections.namedtuple('LossSpec', ['kind', 'weights', 'clim', 'regularize', 'reverse', 'masked'],
                                  defaults=(None, None, None, True, None))


def spec_of(loss):
    """The LossSpec the engine runs for `loss` (a name, one of this module's functions, or a callable of DLWP.custom's loss
    factories), or None when the engine has no kernels for it."""
    if isinstance(loss, str):
        loss = _BY_NAME.get(loss)
    if loss is mean_squared_error:
        return LossSpec('mse')
    if loss is mean_absolute_error:
        return LossSpec('mae')
    return getattr(loss, '_dlwpcs_loss', None)


def config_name(loss):
    """The name keras serialises a loss under: a string as given, a function by its __name__ ('lat_loss', 'acc_loss', ...)."""
    if isinstance(loss, str):
        return loss
    return getattr(loss, '__name__', None)
