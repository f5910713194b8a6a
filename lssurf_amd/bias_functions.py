"""Data biases: one additive offset per unique combination of data fields (sensor, cycle, rgt, …).

Behaviour follows LSsurf/bias_functions.py (assign_bias_ID :25-81, setup_bias_fit :83-115,
parse_biases :118-164) and smooth_fit.py's edit_by_bias (:65-98):

* ``assign_bias_ID`` numbers the unique parameter rows in the order of the reference's
  ``unique_by_rows`` (columns weighted left to right, each by the running product of the earlier
  columns' distinct counts), NaN parameters collapsed into one category and reported back as NaN;
  ``E_bias`` is the nanmedian of ``data.sigma_corr`` per ID.
* ``setup_bias_fit`` appends one column per ID to the data operator (a 1 on each data row in its
  ID's column) and one constraint row per ID, expected value ``E_bias``; a zero raises ValueError.
* ``parse_biases`` reads the biases back out of a model vector; ``edit_by_bias`` removes the data
  of the IDs whose bias is too many expected values from zero.
"""
import numpy as np

from .lin_op import lin_op

NAN_CATEGORY = -9999   # the value NaN parameters share while the rows are compared


def unique_rows(x):
    """The unique rows of x in the reference's order (LSsurf/unique_by_rows.py), and for each the
    indices of the rows of x that equal it (ascending)."""
    x = np.asarray(x)
    if x.ndim == 1:
        x = x.reshape(-1, 1)
    key = np.zeros(x.shape[0])
    scale = 1.
    for col in range(x.shape[1]):
        _, inv = np.unique(x[:, col].astype(np.float64), return_inverse=True)
        scale /= float(np.max(inv)) + 1.
        key += np.ravel(inv) * scale
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    inverse = np.ravel(inverse)
    order = np.argsort(inverse, kind='stable')
    counts = np.bincount(inverse, minlength=first.size)
    groups = np.split(order, np.cumsum(counts)[:-1])
    return x[first, :], groups


def assign_bias_ID(data, bias_params=None, bias_name='bias_ID', key_name=None, bias_filter=None, bias_model=None):
    """Give every datum the ID of the bias that applies to it (field `bias_name` of data) and
    describe the IDs in bias_model: E_bias[ID], bias_ID_dict[ID] = {param: value},
    bias_param_dict = {param: [values…], 'ID': [IDs…]}."""
    if bias_model is None:
        bias_model = {'E_bias': {}, 'bias_param_dict': {}, 'bias_ID_dict': {}}
    first_id = len(bias_model['bias_ID_dict'])
    if bias_params is None:   # one bias for all the data
        bias_model['bias_ID_dict'][first_id + 1] = key_name
        bias_model['E_bias'][first_id + 1] = np.nanmedian(data.sigma_corr)
        data.assign({bias_name: first_id + 1})
        return data, bias_model
    source = bias_filter(data) if bias_filter is not None else data
    table = np.nan_to_num(np.column_stack([getattr(source, p) for p in bias_params]), nan=NAN_CATEGORY)
    rows, groups = unique_rows(table)
    bias_model['bias_param_dict'].update({p: [] for p in bias_params})
    bias_model['bias_param_dict']['ID'] = []
    ids = np.zeros(data.size)
    for k, (row, members) in enumerate(zip(rows, groups)):
        this_id = first_id + k
        reported = row.copy()
        reported[reported == NAN_CATEGORY] = np.nan
        for j, p in enumerate(bias_params):
            bias_model['bias_param_dict'][p].append(row[j])
        bias_model['bias_param_dict']['ID'].append(this_id)
        bias_model['bias_ID_dict'][this_id] = {p: reported[j] for j, p in enumerate(bias_params)}
        bias_model['E_bias'][this_id] = np.nanmedian(data.sigma_corr[members])
        ids[members] = this_id
    data.assign({bias_name: ids})
    return data, bias_model


def bias_expected(bias_model, n_bias):
    """E_bias of IDs 0 … n_bias − 1 as an array; ValueError on a zero."""
    expected = np.array([bias_model['E_bias'][j] for j in range(n_bias)])
    if np.any(expected == 0):
        raise ValueError('found a zero value in the expected biases')
    return expected


def setup_bias_fit(data, bias_model, G_data, constraint_op_list, bias_param_name='data_bias', op_name='data_bias'):
    """Append the bias columns to G_data (right of its columns) and the bias constraint op to
    constraint_op_list; bias_ID_dict[ID]['col'] is the ID's column."""
    ids = getattr(data, bias_param_name).astype(int)
    col_0 = G_data.col_N
    n_bias = int(np.max(ids)) + 1
    col_N = col_0 + n_bias
    G_bias = lin_op(name=op_name, col_0=col_0, col_N=col_N).data_bias(np.arange(data.size), col=col_0 + ids)
    each = np.arange(n_bias, dtype=int)
    Gc_bias = lin_op(name='constraint_' + op_name, col_0=col_0, col_N=col_N).data_bias(each, col=col_0 + each)
    for key in bias_model['bias_ID_dict']:
        bias_model['bias_ID_dict'][key]['col'] = col_0 + key
    Gc_bias.expected = bias_expected(bias_model, n_bias)
    constraint_op_list.append(Gc_bias)
    G_data.add(G_bias)


def parse_biases(m, bias_model, bias_params, data=None):
    """(bias dict, slope-bias dict) of model vector m: per ID its value, expected value and
    parameters, and with data the spread and count of its residuals before and after editing."""
    out = {p: [] for p in list(bias_params) + ['val', 'ID', 'expected']}
    if data is not None:
        out.update({'rms_data_raw': [], 'rms_data_edited': [], 'N_raw': [], 'N_edited': []})
        r = data.z - data.z_est
    for this_id, entry in bias_model['bias_ID_dict'].items():
        out['val'].append(m[entry['col']])
        out['ID'].append(this_id)
        out['expected'].append(bias_model['E_bias'][this_id])
        for p in bias_params:
            out[p].append(entry[p])
        if data is not None:
            mine = data.bias_ID == this_id
            for tag, sel in (('raw', mine), ('edited', mine & (data.three_sigma_edit == 1))):
                rr = r[sel]
                out['rms_data_' + tag].append(np.nanstd(rr) if len(rr) else np.nan)
                out['N_' + tag].append(len(rr))
    slope = {}
    for key, cols in bias_model.get('slope_bias_dict', {}).items():
        slope[key] = {'slope_x': m[cols[0]], 'slope_y': m[cols[1]]}
    return out, slope


def edit_by_bias(data, m0, in_TSE, iteration, bias_model, args):
    """Drop (in in_TSE, in place) the data of the IDs whose bias is beyond bias_nsigma_edit expected
    values — or, when some bias is extreme (beyond min(50, 3 × the 95th percentile)), only the largest
    — from iteration bias_nsigma_iteration on; IDs edited before stay edited.  True when the set of
    edited IDs changed."""
    if args['bias_nsigma_edit'] is None:
        return False
    from scipy.stats import scoreatpercentile
    pd = bias_model['bias_param_dict']
    if 'edited' not in pd:
        pd['edited'] = np.zeros_like(pd['ID'], dtype=bool)
    biases, _ = parse_biases(m0, bias_model, args['bias_params'])
    scaled = np.abs(biases['val']) / np.array(biases['expected'])
    before = pd['edited'].copy()
    bad = before.copy()
    if iteration >= args['bias_nsigma_iteration']:
        extreme = np.minimum(50, 3 * scoreatpercentile(scaled, 95))
        if np.any(scaled > extreme):
            bad[scaled == np.max(scaled)] = True
        else:
            bad[scaled > args['bias_nsigma_edit']] = True
    bad_ids = np.array(biases['ID'])[bad]
    for this_id in bad_ids:
        pd['edited'][pd['ID'].index(this_id)] = True
    if args.get('VERBOSE', True):
        if len(bad_ids):
            print(f'\t have {len(bad_ids)} bad biases, with {np.sum(np.isin(data.bias_ID, bad_ids))} data.')
        elif iteration >= args['bias_nsigma_iteration']:
            print('No bad biases found')
    in_TSE[np.isin(data.bias_ID, bad_ids)] = False
    return bool(~np.all(pd['edited'] == before))
