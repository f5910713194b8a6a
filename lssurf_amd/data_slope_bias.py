"""Slope biases: one tilt in x and one in y per listed sensor (data_slope_sensors).

Behaviour follows LSsurf/data_slope_bias.py (:11-65): of the sensors listed, those present in
data.sensor each get two columns from col_0 on, whose values on the sensor's rows are the x and the
y coordinate minus its nanmean over those rows, in km (so the slopes are in m/km and the columns
stay of order one); bias_model['slope_bias_dict'][sensor] holds the two columns.  The constraint
operator 'constraint_' + op_name has one row per column, expected value E_rms_bias · 1000, prior 0.
"""
import numpy as np

from .lin_op import lin_op

RESCALE = 1000.   # metres per coordinate unit of the slope columns


def slope_columns(data, sensors):
    """(present sensors, group per datum (−1: none), (n, 2) coefficients): the values of the slope
    columns without the operator around them.  Coefficients outside every group are 0."""
    sensors = np.asarray(sensors)
    present = sensors[np.isin(sensors, data.sensor)]
    sensor = np.ravel(data.sensor)
    group = np.full(sensor.size, -1, dtype=np.int32)
    u = np.zeros((sensor.size, 2))
    for k, this in enumerate(present):
        rows = np.flatnonzero(sensor == this)
        group[rows] = k
        for d, var in enumerate(('x', 'y')):
            coord = np.ravel(getattr(data, var))[rows]
            u[rows, d] = (coord - np.nanmean(coord)) / RESCALE
    return present, group, u


def data_slope_bias(data, bias_model, col_0=0, sensors=(), op_name='data_slope', E_rms_bias=1.e-5):
    """(G_slope, Gc_slope, bias_model): the slope columns [col_0, col_0 + 2·(sensors present)) on the
    data rows and their constraint rows; (None, None, bias_model) when no listed sensor is present."""
    present, group, u = slope_columns(data, sensors)
    if len(present) == 0:
        return None, None, bias_model
    slope_dict = bias_model.setdefault('slope_bias_dict', {})
    col_N = col_0 + 2 * len(present)
    for k, this in enumerate(present):
        slope_dict[this] = col_0 + 2 * k + np.array([0, 1])
    # rows by sensor, x column before y column
    in_group = [np.flatnonzero(group == k) for k in range(len(present))]
    G = lin_op(col_0=col_0, col_N=col_N, name=op_name)
    G.r = np.concatenate([rows for rows in in_group for _ in range(2)])
    G.c = np.concatenate([np.full(rows.size, col_0 + 2 * k + d, dtype=int)
                          for k, rows in enumerate(in_group) for d in range(2)])
    G.v = np.concatenate([u[rows, d] for rows in in_group for d in range(2)])
    cols = np.arange(col_0, col_N, dtype=int)
    Gc = lin_op(name='constraint_' + op_name, col_0=col_0, col_N=col_N).data_bias(cols - col_0, col=cols)
    Gc.expected = np.full(cols.size, E_rms_bias * RESCALE)
    Gc.prior = np.zeros(cols.size)
    return G, Gc, bias_model
