#
# MI355X-native counterparts of the reference's custom Keras layers for the cubed sphere.
#

"""
Custom layer classes of the DLWP-CS hot path, same names / constructor signatures / configs / weight order as the
reference module `DLWP/custom.py`, dispatching to hand-written HIP kernels (libdlwpcs.so) instead of TensorFlow:

    CubeSpherePadding2D   reference DLWP/custom.py:1057-1308
    CubeSphereConv2D      reference DLWP/custom.py:755-1054

plus the training callbacks the reference scripts pass to `fit` (reference DLWP/custom.py:33-208), re-hosted on the
TF-free shim in `DLWP.keras`, and the training losses latitude_weighted_loss / anomaly_correlation(_loss) (reference
DLWP/custom.py:1543-1676), which Model.compile runs as HIP kernels, and masked_loss, which lets either of 'mse' / 'mae' ignore
NaN targets.
"""

import numpy as np

from . import ops
from ._native import ACT_LEAKY_CLIP, ACT_NONE
from .keras import constraints, engine, regularizers
from .keras.callbacks import Callback, EarlyStopping
from .keras.engine import Layer
from .keras.losses import LossSpec, mean_absolute_error, mean_squared_error, spec_of


# ==================================================================================================================== #
# helpers mirroring keras' conv_utils
# ==================================================================================================================== #

def _normalize_tuple(value, n, name):
    if isinstance(value, int):
        return (value,) * n
    try:
        value_tuple = tuple(value)
    except TypeError:
        raise ValueError('The `' + name + '` argument must be a tuple of ' + str(n) + ' integers. Received: ' +
                         str(value))
    if len(value_tuple) != n:
        raise ValueError('The `' + name + '` argument must be a tuple of ' + str(n) + ' integers. Received: ' +
                         str(value))
    for single_value in value_tuple:
        try:
            int(single_value)
        except (ValueError, TypeError):
            raise ValueError('The `' + name + '` argument must be a tuple of ' + str(n) + ' integers. Received: ' +
                             str(value) + ' including element ' + str(single_value) + ' of type' + ' ' +
                             str(type(single_value)))
    return tuple(int(v) for v in value_tuple)


def _normalize_data_format(value):
    if value is None:
        value = 'channels_last'
    data_format = value.lower()
    if data_format not in {'channels_first', 'channels_last'}:
        raise ValueError('The `data_format` argument must be one of "channels_first", "channels_last". Received: ' +
                         str(value))
    return data_format


def _normalize_padding(value):
    if isinstance(value, (list, tuple)):
        return value
    padding = value.lower()
    if padding not in {'valid', 'same', 'causal'}:
        raise ValueError('The `padding` argument must be a list/tuple or one of "valid", "same" (or "causal", only for '
                         '`Conv1D). Received: ' + str(padding))
    return padding


def _conv_output_length(input_length, filter_size, padding, stride, dilation=1):
    if input_length is None:
        return None
    dilated_filter_size = filter_size + (filter_size - 1) * (dilation - 1)
    if padding == 'same':
        output_length = input_length
    else:
        output_length = input_length - dilated_filter_size + 1
    return (output_length + stride - 1) // stride


# ==================================================================================================================== #
# Cubed-sphere layers
# ==================================================================================================================== #

class CubeSpherePadding2D(Layer):
    """
    Padding layer for 2D data on a cubed sphere: fills a halo of width `padding` around each of the 6 faces with the
    data of the neighbouring faces (rotated / reversed as the cube geometry requires).

    - input  (batch, channels, 6, height, width) for channels_first, (batch, 6, height, width, channels) for
      channels_last; faces 0-3 are equatorial, 4 and 5 the south and north polar faces
    - output has height and width increased by 2 * padding

    Same constructor, attributes and config as the reference layer (DLWP/custom.py:1072-1080), which derives from
    keras' ZeroPadding3D: `padding` must be an int or a 3-sequence (the reference's default `(1, 1)` raises exactly as
    it does there), and the face axis padding is forced to (0, 0).

    On the device the whole layer is ONE gather through a precomputed table (kernel `pad_fwd_kernel`), and when it is
    followed by a CubeSphereConv2D inside a `DLWP.keras.Model` it is not executed at all: the halo is resolved inside
    the convolution's load.
    """

    def __init__(self, padding=(1, 1), data_format='channels_first', **kwargs):
        data_format = _normalize_data_format(data_format)
        super(CubeSpherePadding2D, self).__init__(**kwargs)
        # --- keras.layers.ZeroPadding3D argument handling ---
        if isinstance(padding, int):
            padding = ((padding, padding), (padding, padding), (padding, padding))
        elif hasattr(padding, '__len__'):
            if len(padding) != 3:
                raise ValueError('`padding` should have 3 elements. Found: ' + str(padding))
            dim1_padding = _normalize_tuple(padding[0], 2, '1st entry of padding')
            dim2_padding = _normalize_tuple(padding[1], 2, '2nd entry of padding')
            dim3_padding = _normalize_tuple(padding[2], 2, '3rd entry of padding')
            padding = (dim1_padding, dim2_padding, dim3_padding)
        else:
            raise ValueError('`padding` should be either an int, a tuple of 3 ints (symmetric_dim1_pad, '
                             'symmetric_dim2_pad, symmetric_dim3_pad), or a tuple of 3 tuples of 2 ints ((left_dim1_pad, '
                             'right_dim1_pad), (left_dim2_pad, right_dim2_pad), (left_dim3_pad, right_dim2_pad)). '
                             'Found: ' + str(padding))
        self.data_format = data_format
        self.padding = ((0, 0),) + tuple(padding[1:])

    def compute_output_shape(self, input_shape):
        input_shape = tuple(input_shape)
        add = [q[0] + q[1] for q in self.padding]
        if self.data_format == 'channels_first':
            dims = [None if input_shape[2 + i] is None else input_shape[2 + i] + add[i] for i in range(3)]
            return (input_shape[0], input_shape[1]) + tuple(dims)
        dims = [None if input_shape[1 + i] is None else input_shape[1 + i] + add[i] for i in range(3)]
        return (input_shape[0],) + tuple(dims) + (input_shape[4],)

    def call(self, inputs):
        p = self.padding[1][0]
        if self.data_format == 'channels_first':
            x = ops.channels_first_to_last(inputs)
            return ops.channels_last_to_first(ops.cs_pad(x, p))
        return ops.cs_pad(inputs, p)

    def get_config(self):
        config = {'padding': self.padding, 'data_format': self.data_format}
        base_config = super(CubeSpherePadding2D, self).get_config()
        return dict(list(base_config.items()) + list(config.items()))


class CubeSphereConv2D(Layer):
    """
    2D convolutional layer for data on a cubed sphere.

    - input (batch, channels, 6, height, width) for channels_first, (batch, 6, height, width, channels) for
      channels_last; the last two faces (4, 5) are the polar faces
    - learns one kernel + bias for the four equatorial faces and one for the polar faces; optionally a third set for
      the north pole (`independent_north_pole`); with `flip_north_pole` the north-pole face is convolved in the
      south pole's orientation (rows reversed before and after)
    - should be preceded by CubeSpherePadding2D, otherwise faces are not connected

    Same constructor signature, attributes, `get_config()` keys and weight creation order as the reference
    (DLWP/custom.py:824-919,1032-1054): equatorial_kernel, polar_kernel, [north_pole_kernel], equatorial_bias,
    polar_bias, [north_pole_bias], kernels in HWIO layout.

    Device path: the hot configuration (kernel 3 or 1, stride 1, dilation 1, 'valid') runs on the MFMA implicit-GEMM
    kernel `conv_mfma_kernel`; the pole weight sharing is a per-face choice of packed weight variant, the north-pole
    flip a row-reversed kernel variant (no data is moved).  Other options run on the generic direct kernels.
    """

    def __init__(self,
                 filters,
                 kernel_size,
                 strides=1,
                 padding='valid',
                 data_format='channels_first',
                 dilation_rate=1,
                 activation=None,
                 use_bias=True,
                 flip_north_pole=True,
                 independent_north_pole=False,
                 kernel_initializer='glorot_uniform',
                 bias_initializer='zeros',
                 kernel_regularizer=None,
                 bias_regularizer=None,
                 activity_regularizer=None,
                 kernel_constraint=None,
                 bias_constraint=None,
                 **kwargs):
        super(CubeSphereConv2D, self).__init__(**kwargs)
        self.filters = filters
        self.kernel_size = _normalize_tuple(kernel_size, 2, 'kernel_size')
        self.strides = _normalize_tuple(strides, 2, 'strides')
        self.padding = _normalize_padding(padding)
        self.data_format = _normalize_data_format(data_format)
        self.dilation_rate = _normalize_tuple(dilation_rate, 2, 'dilation_rate')
        self.activation = engine.get_activation(activation)
        self.use_bias = use_bias
        self.flip_north_pole = flip_north_pole
        self.independent_north_pole = independent_north_pole
        self.kernel_initializer = engine.get_initializer(kernel_initializer)
        self.bias_initializer = engine.get_initializer(bias_initializer)
        self.kernel_regularizer = regularizers.get(kernel_regularizer)
        self.bias_regularizer = regularizers.get(bias_regularizer)
        self.activity_regularizer = engine._passthrough_get(activity_regularizer)
        self.kernel_constraint = constraints.get(kernel_constraint)
        self.bias_constraint = constraints.get(bias_constraint)
        self.rank = 3

        self.equatorial_kernel = None
        self.equatorial_bias = None
        self.polar_kernel = None
        self.polar_bias = None
        self.north_pole_kernel = None
        self.north_pole_bias = None

    def _weight_attr_names(self):
        return ['equatorial_kernel', 'polar_kernel', 'north_pole_kernel', 'equatorial_bias', 'polar_bias',
                'north_pole_bias']

    def build(self, input_shape):
        if self.data_format == 'channels_first':
            channel_axis = 1
        else:
            channel_axis = -1
        if input_shape[channel_axis] is None:
            raise ValueError('The channel dimension of the inputs should be defined. Found `None`.')
        input_dim = int(input_shape[channel_axis])
        kernel_shape = self.kernel_size + (input_dim, self.filters)

        self.equatorial_kernel = self.add_weight(shape=kernel_shape, initializer=self.kernel_initializer,
                                                 name='equatorial_kernel', regularizer=self.kernel_regularizer,
                                                 constraint=self.kernel_constraint)
        self.polar_kernel = self.add_weight(shape=kernel_shape, initializer=self.kernel_initializer,
                                            name='polar_kernel', regularizer=self.kernel_regularizer,
                                            constraint=self.kernel_constraint)
        if self.independent_north_pole:
            self.north_pole_kernel = self.add_weight(shape=kernel_shape, initializer=self.kernel_initializer,
                                                     name='north_pole_kernel', regularizer=self.kernel_regularizer,
                                                     constraint=self.kernel_constraint)
        if self.use_bias:
            self.equatorial_bias = self.add_weight(shape=(self.filters,), initializer=self.bias_initializer,
                                                   name='equatorial_bias', regularizer=self.bias_regularizer,
                                                   constraint=self.bias_constraint)
            self.polar_bias = self.add_weight(shape=(self.filters,), initializer=self.bias_initializer,
                                              name='polar_bias', regularizer=self.bias_regularizer,
                                              constraint=self.bias_constraint)
            if self.independent_north_pole:
                self.north_pole_bias = self.add_weight(shape=(self.filters,), initializer=self.bias_initializer,
                                                       name='north_pole_bias', regularizer=self.bias_regularizer,
                                                       constraint=self.bias_constraint)
        self.input_dim = input_dim
        self.built = True

    # ------------------------------------------------------------------------------------------------------------ #
    def _is_mfma_config(self):
        k = self.kernel_size
        return (k[0] == k[1] and k[0] in (1, 3) and self.strides == (1, 1) and self.dilation_rate == (1, 1)
                and self.padding == 'valid')

    def can_fuse_halo(self, pad_width):
        """True if a preceding CubeSpherePadding2D(pad_width) can be folded into this layer's load."""
        return (self._is_mfma_config() and self.kernel_size[0] == 3 and pad_width == 1 and self.activation is None)

    def fused_call(self, src0, src1=None, up0=False, halo=True, act=ACT_NONE, alpha=0.0, vmax=0.0, premask0=None,
                   premask1=None, dy_premasked=False, defer_ring0=False, want_pool=False, out_padded=False, small=False):
        """pad -> conv (-> ReLU) with optional upsample/concat on the input side, as one kernel (channels_last).
        premask0 / premask1 / dy_premasked: the pre-masked gradient convention of the training step (ops._CSConv).
        small: engine option small_conv (ops.cs_conv)."""
        return ops.cs_conv(src0, self.equatorial_kernel, self.polar_kernel, self.north_pole_kernel,
                           self.equatorial_bias, self.polar_bias, self.north_pole_bias, src1=src1,
                           ksize=self.kernel_size[0], halo=halo, up0=up0, flip_north_pole=self.flip_north_pole,
                           act=act, alpha=alpha, vmax=vmax, premask0=premask0, premask1=premask1,
                           dy_premasked=dy_premasked, defer_ring0=defer_ring0, want_pool=want_pool, out_padded=out_padded,
                           small=small)

    def call(self, inputs, channels_last_io=False, **kwargs):
        """channels_last_io (DLWP.keras.Model running a channels_first graph channels_last inside): the tensor arrives and
        leaves channels_last whatever the layer's data_format says."""
        channels_first = self.data_format == 'channels_first' and not channels_last_io
        x = ops.channels_first_to_last(inputs) if channels_first else inputs
        if self._is_mfma_config():
            outputs = ops.cs_conv(x, self.equatorial_kernel, self.polar_kernel, self.north_pole_kernel,
                                  self.equatorial_bias, self.polar_bias, self.north_pole_bias,
                                  ksize=self.kernel_size[0], halo=False, flip_north_pole=self.flip_north_pole)
        else:
            outputs = ops.cs_gconv(x, self.equatorial_kernel, self.polar_kernel, self.north_pole_kernel,
                                   self.equatorial_bias, self.polar_bias, self.north_pole_bias,
                                   strides=self.strides, padding=self.padding, dilation=self.dilation_rate,
                                   flip_north_pole=self.flip_north_pole)
        if channels_first:
            outputs = ops.channels_last_to_first(outputs)
        if self.activation is not None:
            return self.activation(outputs)
        return outputs

    def compute_output_shape(self, input_shape):
        if self.data_format == 'channels_last':
            # batch, face, height, width, ...
            space = input_shape[2:4]
        else:
            # batch, channels, face, height, width
            space = input_shape[-2:]
        new_space = []
        for i in range(len(space)):
            new_space.append(_conv_output_length(space[i], self.kernel_size[i], padding=self.padding,
                                                 stride=self.strides[i], dilation=self.dilation_rate[i]))
        if self.data_format == 'channels_last':
            return (input_shape[0], 6) + tuple(new_space) + (self.filters,)
        return (input_shape[0], self.filters, 6) + tuple(new_space)

    def get_config(self):
        config = {
            'filters': self.filters,
            'kernel_size': self.kernel_size,
            'strides': self.strides,
            'padding': self.padding,
            'data_format': self.data_format,
            'dilation_rate': self.dilation_rate,
            'activation': engine.serialize_activation(self.activation),
            'use_bias': self.use_bias,
            'flip_north_pole': self.flip_north_pole,
            'independent_north_pole': self.independent_north_pole,
            'kernel_initializer': engine.serialize_initializer(self.kernel_initializer),
            'bias_initializer': engine.serialize_initializer(self.bias_initializer),
            'kernel_regularizer': regularizers.serialize(self.kernel_regularizer),
            'bias_regularizer': regularizers.serialize(self.bias_regularizer),
            'activity_regularizer': self.activity_regularizer,
            'kernel_constraint': constraints.serialize(self.kernel_constraint),
            'bias_constraint': constraints.serialize(self.bias_constraint)
        }
        base_config = super(CubeSphereConv2D, self).get_config()
        return dict(list(base_config.items()) + list(config.items()))


# ==================================================================================================================== #
# Training callbacks used by the cubed-sphere scripts (behaviour of reference DLWP/custom.py:33-208)
# ==================================================================================================================== #

def _adam_effective_lr(optimizer, beta_1, beta_2, with_bias_correction):
    it = float(optimizer.iterations)
    lr = float(optimizer.lr) / (1. + float(getattr(optimizer, 'decay', 0.)) * it)
    if with_bias_correction:
        t = it + 1.
        lr = lr * np.sqrt(1. - np.power(beta_2, t)) / (1. - np.power(beta_1, t))
    return lr


class AdamLearningRateTracker(Callback):
    """Prints the bias-corrected Adam step size at the end of each epoch (reference DLWP/custom.py:33-46)."""

    def on_epoch_end(self, epoch, logs=None, beta_1=0.9, beta_2=0.999, ):
        print(' - LR: {:.6f}'.format(_adam_effective_lr(self.model.optimizer, beta_1, beta_2, True)))


class SGDLearningRateTracker(Callback):
    """Prints the decayed learning rate at the end of each epoch (reference DLWP/custom.py:49-60)."""

    def on_epoch_end(self, epoch, logs=None):
        print(' - LR: {:.6f}'.format(_adam_effective_lr(self.model.optimizer, 0., 0., False)))


class BatchHistory(Callback):
    """Collects the per-batch logs, one dict of lists per epoch (reference DLWP/custom.py:63-81)."""

    def on_train_begin(self, logs=None):
        self.history, self.epoch = [], 0

    def on_epoch_begin(self, epoch, logs=None):
        self.history.append(dict())

    def on_batch_end(self, batch, logs=None):
        for key, value in (logs or {}).items():
            self.history[self.epoch].setdefault(key, []).append(value)

    def on_epoch_end(self, epoch, logs=None):
        self.epoch += 1


class RunHistory(Callback):
    """keras `History` that additionally forwards every epoch value to `run.log(key, value)` (an AzureML `Run`;
    reference DLWP/custom.py:84-105)."""

    def __init__(self, run):
        super(RunHistory, self).__init__()
        self.run = run
        self.epoch, self.history = [], {}

    def on_train_begin(self, logs=None):
        self.epoch, self.history = [], {}

    def on_epoch_end(self, epoch, logs=None):
        self.epoch.append(epoch)
        for key, value in (logs or {}).items():
            self.history.setdefault(key, []).append(value)
            self.run.log(key, value)


class RNNResetStates(Callback):
    """Resets recurrent states when an epoch begins (reference DLWP/custom.py:108-110); no-op for the CNN."""

    def on_epoch_begin(self, epoch, logs=None):
        self.model.reset_states()


class EarlyStoppingMin(EarlyStopping):
    """
    EarlyStopping that ignores the first `min_epochs` epochs entirely and stops unconditionally once `max_epochs` is
    reached, restoring the best weights in both cases when asked to (reference DLWP/custom.py:113-165).
    """

    def __init__(self, min_epochs=0, max_epochs=None, **kwargs):
        super(EarlyStoppingMin, self).__init__(**kwargs)
        if not isinstance(min_epochs, int) or min_epochs < 0:
            raise ValueError('min_epochs must be an integer >= 0')
        self.min_epochs = int(min_epochs)
        self.max_epochs = None if max_epochs is None else int(max_epochs)

    def _stop(self, epoch, message):
        self.stopped_epoch = epoch
        self.model.stop_training = True
        if self.restore_best_weights:
            if self.verbose > 0:
                print(message)
            self.model.set_weights(self.best_weights)

    def on_epoch_end(self, epoch, logs=None):
        if epoch < self.min_epochs:
            return
        current = self.get_monitor_value(logs)
        if current is None:
            return
        improved = self.monitor_op(current - self.min_delta, self.best)
        if improved:
            self.best, self.wait = current, 0
            if self.restore_best_weights:
                self.best_weights = self.model.get_weights()
        else:
            self.wait += 1
            if self.wait >= self.patience:
                self._stop(epoch, 'Restoring model weights from the end of the best epoch')
        if self.max_epochs is not None and epoch >= self.max_epochs:
            self._stop(epoch, 'Maximum epochs reached; restoring model weights from the end of the best epoch')
        if self.verbose > 1:
            print('EarlyStoppingMin: %d epochs since last minimum' % self.wait)


class SaveWeightsOnEpoch(Callback):
    """
    Writes the weights to `weights_file` after every epoch (I/O errors are swallowed so a locked file cannot kill a
    run); on every `interval`-th epoch the snapshot goes to `weights_file.<epoch>` instead
    (reference DLWP/custom.py:168-191).
    """

    def __init__(self, weights_file, interval=None):
        super(SaveWeightsOnEpoch, self).__init__()
        self.weights_file = str(weights_file)
        if interval is not None:
            assert isinstance(interval, int) and interval > 0, "'interval' must be an integer > 0"
        self.interval = interval

    def on_epoch_end(self, epoch, logs=None):
        if self.interval is not None and epoch % self.interval == 0:
            self.model.save_weights('%s.%s' % (self.weights_file, epoch), save_format='h5')
            return
        try:
            self.model.save_weights(self.weights_file, save_format='h5')
        except OSError:
            pass


class GeneratorEpochEnd(Callback):
    """Runs `generator.on_epoch_end()` (re-shuffle) after each epoch when the data are fed through a dataset wrapper
    that hides the generator from the training loop (reference DLWP/custom.py:194-208)."""

    def __init__(self, generator):
        super(GeneratorEpochEnd, self).__init__()
        self.generator = generator

    def on_epoch_end(self, epoch, logs=None):
        self.generator.on_epoch_end()


# ==================================================================================================================== #
# Keras loss functions (reference DLWP/custom.py:1543-1676)
# ==================================================================================================================== #
# Host callables with the reference's semantics (numpy or torch arrays in, keras' loss value out).  Each carries a
# `_dlwpcs_loss` spec (DLWP.keras.losses.LossSpec): Model.compile reads it and runs the HIP loss kernels (DLWP.ops.loss_stats)
# in its place -- a callable without one is refused there.


def _xp_like(a, ref):
    """a (numpy / scalar) as an array of ref's kind (torch: same device and dtype)"""
    if hasattr(ref, 'detach') and not hasattr(a, 'detach'):
        import torch
        return torch.as_tensor(np.asarray(a), dtype=ref.dtype, device=ref.device)
    return a


def _mean(x, axis=None):
    if hasattr(x, 'detach'):
        return x.mean() if axis is None else x.mean(dim=tuple(axis))
    return np.mean(x) if axis is None else np.mean(x, axis=tuple(axis))


def _sqrt(x):
    return x.sqrt() if hasattr(x, 'detach') else np.sqrt(x)


def _abs(x):
    return x.abs() if hasattr(x, 'detach') else np.abs(x)


def latitude_weighted_loss(loss_function=mean_squared_error, lats=None, output_shape=(), axis=-2, weighting='cosine'):
    """
    Create a loss function that weights inputs by a function of latitude before calculating the loss (reference
    DLWP/custom.py:1543-1578, same signature, defaults and errors).

    The weight field is cos(lat), or cos(lat) + 0.5 sin^2(2 lat) for 'midlatitude', expanded and repeated over
    output_shape[axis:][1:]; ones(output_shape) without `lats`.  The loss is loss_function(y_true * w, y_pred * w): w enters a
    mean squared error SQUARED (mean(w^2 (y_pred - y_true)^2)) -- the reference's definition, kept as is.

    On the cubed sphere pass the grid's per-cell latitudes, ds.lat of shape (6, N, N), with output_shape (6, N, N, C) and
    axis=-2 (channels_last): the field becomes (6, N, N, C).  A channels_first output (C, 6, N, N) takes axis=-1 (field
    (6, N, N), broadcast over the channels).

    :param loss_function: mean_squared_error / mean_absolute_error (DLWP.keras.losses) or an anomaly-correlation loss of
        this module -- the forms the DLWP-CS engine runs on the GPU
    :param lats: ndarray: latitude coordinates (degrees)
    :param output_shape: tuple: shape of expected model output
    :param axis: int: latitude axis in model output shape
    :param weighting: str: 'cosine' (default) or 'midlatitude'
    :return: callable loss function `lat_loss`
    """
    if weighting not in ['cosine', 'midlatitude']:
        raise ValueError("'weighting' must be one of 'cosine' or 'midlatitude'")
    if lats is not None:
        lat = np.asarray(lats[:]).astype(np.float32)
        weights = np.cos(lat * np.pi / 180.)
        if weighting == 'midlatitude':
            weights = weights + 0.5 * np.power(np.sin(lat * 2 * np.pi / 180.), 2.)
        weight_shape = tuple(output_shape)[axis:]
        for d in weight_shape[1:]:
            weights = np.expand_dims(weights, axis=-1)
            weights = np.repeat(weights, d, axis=-1)
    else:
        weights = np.ones(output_shape, dtype=np.float32)
    weights = weights.astype(np.float32)

    def lat_loss(y_true, y_pred):
        w = _xp_like(weights, y_pred)
        return loss_function(y_true * w, y_pred * w)

    inner = spec_of(loss_function)
    lat_loss._dlwpcs_loss = None if (inner is None or inner.weights is not None) else inner._replace(weights=weights)
    lat_loss.weights = weights
    return lat_loss


def _acc_value(y_true, y_pred, mean, regularize_mean, reverse):
    if mean is not None:
        mean = _xp_like(mean, y_pred)
        a = (_mean((y_pred - mean) * (y_true - mean))
             / _sqrt(_mean((y_pred - mean) ** 2) * _mean((y_true - mean) ** 2)))
    else:
        a = _mean(y_pred * y_true) / _sqrt(_mean(y_pred ** 2) * _mean(y_true ** 2))
    if regularize_mean is not None:
        if regularize_mean == 'global':
            m = _abs((_mean(y_true) - _mean(y_pred)) / _mean(y_true))
        elif regularize_mean == 'spatial':
            m = _mean(_abs((_mean(y_true, axis=[-2, -1]) - _mean(y_pred, axis=[-2, -1])) / _mean(y_true, axis=[-2, -1])))
        elif regularize_mean == 'mse':
            m = mean_squared_error(y_true, y_pred)          # (per row, like the reference: keras' reduction averages it)
        else:
            m = mean_absolute_error(y_true, y_pred)
    if reverse:
        return m - a if regularize_mean is not None else -a
    return a - m if regularize_mean else a


def anomaly_correlation(y_true, y_pred, mean=0., regularize_mean='mse', reverse=True):
    """
    Anomaly correlation (reference DLWP/custom.py:1581-1620): `mean` is IGNORED, as in the reference (the climatology is
    assumed to be 0); regularize_mean in {None, 'global', 'spatial', 'mse', 'mae'}; reverse: -1 is the target score.
    """
    if regularize_mean is not None:
        assert regularize_mean in ['global', 'spatial', 'mse', 'mae']
    return _acc_value(y_true, y_pred, None, regularize_mean, reverse)


anomaly_correlation._dlwpcs_loss = LossSpec('acc', None, None, 'mse', True)


def anomaly_correlation_loss(mean=None, regularize_mean='mse', reverse=True):
    """
    Keras loss function `acc_loss` for the anomaly correlation (reference DLWP/custom.py:1623-1676).

    :param mean: ndarray or None: climatology, the shape of the prediction with a batch axis of 1
    :param regularize_mean: None, 'global', 'spatial', 'mse' or 'mae' (with a regulariser, reverse is forced to True).
        The DLWP-CS engine trains every form but 'spatial' (a per-sample reduction over the layout's last two axes).
    :param reverse: bool: if True, inverts the loss so that -1 is the (minimized) target score
    """
    if mean is not None:
        assert len(mean.shape) > 1
        assert mean.shape[0] == 1
        mean = np.asarray(mean, dtype=np.float32)
    if regularize_mean is not None:
        assert regularize_mean in ['global', 'spatial', 'mse', 'mae']
        reverse = True

    def acc_loss(y_true, y_pred):
        return _acc_value(y_true, y_pred, mean, regularize_mean, reverse)

    acc_loss._dlwpcs_loss = LossSpec('acc', None, mean, regularize_mean, bool(reverse))
    return acc_loss


# ==================================================================================================================== #
# Losses for targets with holes (no counterpart in the reference)
# ==================================================================================================================== #

def _inner_of_masked(loss_function):
    """the LossSpec masked_loss wraps: 'mse' / 'mae' by name or function, or a latitude_weighted_loss of either"""
    inner = spec_of(loss_function)
    if inner is not None and inner.kind == 'acc':
        raise NotImplementedError('masked_loss: a masked anomaly-correlation loss is not built (its sums run over the whole '
                                  'batch: a hole would have to leave all of them)')
    if inner is None or inner.kind not in ('mse', 'mae') or inner.masked is not None:
        raise ValueError("masked_loss wraps 'mse' / 'mae' (DLWP.keras.losses, by name or function) or a latitude_weighted_loss "
                         "of either, got %r" % (loss_function,))
    return inner


def masked_loss(loss_function=mean_squared_error, normalize='valid'):
    """
    Create a loss function that ignores the elements whose TARGET is NaN (a field with holes: sea-surface temperature over
    land).  An element is a hole iff y_true is NaN there; y_pred is never inspected, and at a hole it contributes nothing --
    neither to the loss nor to the gradient (which is 0 there), whatever its value.  +-inf targets are data.

    :param loss_function: 'mse' / 'mae', mean_squared_error / mean_absolute_error (DLWP.keras.losses), or the result of
        latitude_weighted_loss(...) of either
    :param normalize: 'valid' (default): the sum of the terms divided by the number of valid elements of the batch (a nan-mean;
        0 when nothing is valid); 'all': divided by the number of all elements, i.e. a hole counts as a perfect prediction.
        The weighted forms divide by the same number (the weight field has mean 1).  'all' is exact under data-parallel
        averaging; 'valid' is refused there (per-rank nan-means averaged over ranks are a different loss).
    :return: callable loss function `masked_loss`.  On host arrays (numpy or torch) it returns an array of y_pred's shape
        without the last axis whose plain mean is the loss, so that keras' reduction over the rest gives the value.
    """
    if normalize not in ('all', 'valid'):
        raise ValueError("'normalize' must be one of 'all' or 'valid'")
    inner = _inner_of_masked(loss_function)
    weights = inner.weights

    def masked_loss(y_true, y_pred):
        hole = y_true != y_true
        if hasattr(y_pred, 'detach'):
            import torch
            d = torch.where(hole, torch.zeros_like(y_pred), y_pred - y_true)      # (a select: a NaN y_pred at a hole is dropped)
        else:
            d = np.where(hole, 0., y_pred - y_true)
        if weights is not None:
            d = d * _xp_like(weights, y_pred)
        term = d * d if inner.kind == 'mse' else _abs(d)
        rows = term.sum(-1)
        if normalize == 'all':
            return rows / y_pred.shape[-1]
        count = (~hole).sum()
        n_rows = max(int(np.prod(tuple(rows.shape))), 1)
        if int(count) == 0:
            return rows * 0
        if hasattr(count, 'detach'):
            return rows * (n_rows / count.to(rows.dtype))       # (an integer tensor would divide in float32)
        return rows * rows.dtype.type(n_rows / float(count))

    masked_loss._dlwpcs_loss = inner._replace(masked=normalize)
    masked_loss.normalize = normalize
    return masked_loss
