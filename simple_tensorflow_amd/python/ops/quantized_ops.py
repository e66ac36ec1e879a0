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


def quantized_conv2d_with_bias_and_requantize(
        input, filter, bias, min_input, max_input,  # noqa: A002
        min_filter, max_filter, requested_output_min, requested_output_max,
        strides, padding, activation='None', name=None):
    """quantized_conv2d, a float bias [cout], activation ('None', 'Relu' or
    'Relu6') and the quantization to [requested_output_min,
    requested_output_max] in one op -> (quint8 output, min_output,
    max_output): out = quantize(activation(float(acc) * step_input *
    step_filter + bias)), all in f32."""
    return apply_op('QuantizedConv2DWithBiasAndRequantize', input, filter,
                    convert_to_tensor(bias, dtype=dtypes.float32),
                    convert_to_tensor(min_input),
                    convert_to_tensor(max_input),
                    convert_to_tensor(min_filter),
                    convert_to_tensor(max_filter),
                    convert_to_tensor(requested_output_min),
                    convert_to_tensor(requested_output_max),
                    strides=list(strides), padding=padding,
                    activation=activation, name=name)


def quantized_conv2d_with_bias_sum_and_requantize(
        input, filter, bias, summand, min_input, max_input,  # noqa: A002
        min_filter, max_filter, min_summand, max_summand,
        requested_output_min, requested_output_max, strides, padding,
        activation='None', name=None):
    """quantized_conv2d_with_bias_and_requantize with a residual sum in
    front of the activation: summand is a quint8 tensor of exactly the
    output's shape [N, P, Q, cout] (no broadcasting) under [min_summand,
    max_summand]. out = quantize(activation(float(acc) * step_input *
    step_filter + bias + dequantize(summand))), all in f32."""
    return apply_op('QuantizedConv2DWithBiasSumAndRequantize', input, filter,
                    convert_to_tensor(bias, dtype=dtypes.float32), summand,
                    convert_to_tensor(min_input),
                    convert_to_tensor(max_input),
                    convert_to_tensor(min_filter),
                    convert_to_tensor(max_filter),
                    convert_to_tensor(min_summand),
                    convert_to_tensor(max_summand),
                    convert_to_tensor(requested_output_min),
                    convert_to_tensor(requested_output_max),
                    strides=list(strides), padding=padding,
                    activation=activation, name=name)


def quantized_depthwise_conv2d(input, filter, min_input,  # noqa: A002
                               max_input, min_filter, max_filter, strides,
                               padding, name=None):
    """NHWC quint8 input, [R,S,C,mult] quint8 filter -> (qint32 output
    [N,P,Q,C*mult], min_output, max_output). strides = [1, sh, sw, 1]."""
    return apply_op('QuantizedDepthwiseConv2D', input, filter,
                    convert_to_tensor(min_input),
                    convert_to_tensor(max_input),
                    convert_to_tensor(min_filter),
                    convert_to_tensor(max_filter), strides=list(strides),
                    padding=padding, name=name)


def quantized_depthwise_conv2d_with_bias_and_requantize(
        input, filter, bias, min_input, max_input,  # noqa: A002
        min_filter, max_filter, requested_output_min, requested_output_max,
        strides, padding, activation='None', name=None):
    """quantized_depthwise_conv2d, a float bias [C*mult], activation and the
    quantization to the requested range in one op -> (quint8 output,
    min_output, max_output); see quantized_conv2d_with_bias_and_requantize."""
    return apply_op('QuantizedDepthwiseConv2DWithBiasAndRequantize', input,
                    filter, convert_to_tensor(bias, dtype=dtypes.float32),
                    convert_to_tensor(min_input),
                    convert_to_tensor(max_input),
                    convert_to_tensor(min_filter),
                    convert_to_tensor(max_filter),
                    convert_to_tensor(requested_output_min),
                    convert_to_tensor(requested_output_max),
                    strides=list(strides), padding=padding,
                    activation=activation, name=name)


def quantized_matmul_with_bias_and_requantize(
        a, b, bias, min_a, max_a, min_b, max_b, requested_output_min,
        requested_output_max, transpose_a=False, transpose_b=False,
        activation='None', name=None):
    """quantized_matmul with a float bias [N], activation and the
    quantization to the requested range in one op -> (quint8 out, min_out,
    max_out); see quantized_conv2d_with_bias_and_requantize."""
    return apply_op('QuantizedMatMulWithBiasAndRequantize', a, b,
                    convert_to_tensor(bias, dtype=dtypes.float32),
                    convert_to_tensor(min_a), convert_to_tensor(max_a),
                    convert_to_tensor(min_b), convert_to_tensor(max_b),
                    convert_to_tensor(requested_output_min),
                    convert_to_tensor(requested_output_max),
                    transpose_a=transpose_a, transpose_b=transpose_b,
                    activation=activation, name=name)


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
            'QuantizedConv2D', 'QuantizedConv2DWithBiasAndRequantize',
            'QuantizedConv2DWithBiasSumAndRequantize',
            'QuantizedDepthwiseConv2D',
            'QuantizedDepthwiseConv2DWithBiasAndRequantize',
            'QuantizedMatMulWithBiasAndRequantize',
            'QuantizeDownAndShrinkRange', 'RequantizationRange',
            'Requantize', 'QuantizedBiasAdd', 'QuantizedMaxPool',
            'QuantizedAvgPool', 'QuantizedRelu6', 'QuantizedConcat',
            'QuantizedReshape'):
    NoGradient(_op)
