"""Quantized ops (reference array_ops quantize section; kernels in
csrc/kernels/cpu_quantized.cc and, on the GPU, csrc/kernels/gpu_quantized.cc
— quint8/qint32 carried as uint8/int32)."""
from simple_tensorflow_amd.python.framework import dtypes
from simple_tensorflow_amd.python.framework.ops import (
    NoGradient, apply_op, convert_to_tensor)


def quantize_v2(input, min_range, max_range, T=dtypes.uint8,  # noqa: A002
                mode='MIN_COMBINED', name=None):
    return apply_op('QuantizeV2',
                    convert_to_tensor(input, dtype=dtypes.float32),
                    convert_to_tensor(float(min_range)),
                    convert_to_tensor(float(max_range)), mode=mode,
                    name=name)


def dequantize(input, min_range, max_range, mode='MIN_COMBINED',  # noqa: A002
               name=None):
    return apply_op('Dequantize', convert_to_tensor(input),
                    convert_to_tensor(min_range),
                    convert_to_tensor(max_range), mode=mode, name=name)


def quantized_matmul(a, b, min_a, max_a, min_b, max_b, transpose_a=False,
                     transpose_b=False, name=None):
    return apply_op('QuantizedMatMul', a, b, convert_to_tensor(min_a),
                    convert_to_tensor(max_a), convert_to_tensor(min_b),
                    convert_to_tensor(max_b), transpose_a=transpose_a,
                    transpose_b=transpose_b, name=name)


def quantized_conv2d(input, filter, min_input, max_input,  # noqa: A002
                     min_filter, max_filter, strides, padding, name=None):
    """NHWC quint8 input, [R,S,C,K] quint8 filter -> (qint32 output,
    min_output, max_output). strides = [1, sh, sw, 1]."""
    return apply_op('QuantizedConv2D', input, filter,
                    convert_to_tensor(min_input),
                    convert_to_tensor(max_input),
                    convert_to_tensor(min_filter),
                    convert_to_tensor(max_filter), strides=list(strides),
                    padding=padding, name=name)


def quantized_relu(features, min_features, max_features, name=None):
    return apply_op('QuantizedRelu', features,
                    convert_to_tensor(min_features),
                    convert_to_tensor(max_features), name=name)


def quantize_down_and_shrink_range(input, input_min, input_max,  # noqa: A002
                                   name=None):
    return apply_op('QuantizeDownAndShrinkRange', input,
                    convert_to_tensor(input_min),
                    convert_to_tensor(input_max), name=name)


def requantization_range(input, input_min, input_max, name=None):  # noqa: A002
    return apply_op('RequantizationRange', input,
                    convert_to_tensor(input_min),
                    convert_to_tensor(input_max), name=name)


def requantize(input, input_min, input_max,  # noqa: A002
               requested_output_min, requested_output_max, name=None):
    """qint32 -> (quint8 output, output_min, output_max) over the requested
    range: QuantizeDownAndShrinkRange without the min/max pass."""
    return apply_op('Requantize', input, convert_to_tensor(input_min),
                    convert_to_tensor(input_max),
                    convert_to_tensor(requested_output_min),
                    convert_to_tensor(requested_output_max), name=name)


def quantized_bias_add(input, bias, min_input, max_input,  # noqa: A002
                       min_bias, max_bias, name=None):
    """quint8 [..., C] + quint8 [C] -> (qint32 output, min_out, max_out)."""
    return apply_op('QuantizedBiasAdd', input, bias,
                    convert_to_tensor(min_input),
                    convert_to_tensor(max_input),
                    convert_to_tensor(min_bias),
                    convert_to_tensor(max_bias), name=name)


def quantized_max_pool(input, min_input, max_input, ksize,  # noqa: A002
                       strides, padding, name=None):
    """NHWC quint8 -> (quint8 output, min_output, max_output)."""
    return apply_op('QuantizedMaxPool', input, convert_to_tensor(min_input),
                    convert_to_tensor(max_input), ksize=list(ksize),
                    strides=list(strides), padding=padding, name=name)


def quantized_avg_pool(input, min_input, max_input, ksize,  # noqa: A002
                       strides, padding, name=None):
    """NHWC quint8 -> (quint8 output, min_output, max_output): the sum of
    the taps inside the image over their number, in integer division."""
    return apply_op('QuantizedAvgPool', input, convert_to_tensor(min_input),
                    convert_to_tensor(max_input), ksize=list(ksize),
                    strides=list(strides), padding=padding, name=name)


def quantized_relu6(features, min_features, max_features, name=None):
    return apply_op('QuantizedRelu6', features,
                    convert_to_tensor(min_features),
                    convert_to_tensor(max_features), name=name)


def quantized_concat(concat_dim, values, input_mins, input_maxes, name=None):
    """N quint8 tensors with a range each -> (quint8 output, output_min,
    output_max) over [min(0, min of the mins), max of the maxes]."""
    return apply_op('QuantizedConcat',
                    convert_to_tensor(concat_dim, dtype=dtypes.int32),
                    list(values),
                    [convert_to_tensor(m) for m in input_mins],
                    [convert_to_tensor(m) for m in input_maxes], name=name)


def quantized_reshape(tensor, shape, input_min, input_max, name=None):
    return apply_op('QuantizedReshape', tensor,
                    convert_to_tensor(shape, dtype=dtypes.int32),
                    convert_to_tensor(input_min),
                    convert_to_tensor(input_max), name=name)


for _op in ('QuantizeV2', 'Dequantize', 'QuantizedMatMul', 'QuantizedRelu',
            'QuantizedConv2D',
            'QuantizeDownAndShrinkRange', 'RequantizationRange',
            'Requantize', 'QuantizedBiasAdd', 'QuantizedMaxPool',
            'QuantizedAvgPool', 'QuantizedRelu6', 'QuantizedConcat',
            'QuantizedReshape'):
    NoGradient(_op)
