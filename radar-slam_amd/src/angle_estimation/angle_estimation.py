"""Angle-of-arrival estimation (MUSIC / ESPRIT / beamforming) on MI355X.

Drop-in for ``src/angle_estimation/angle_estimation.py`` of the reference (``AngleEstimator`` :23-365,
``extract_angles_from_rds`` :368-417).

The reference's MUSIC covariance is rank-1 (R = s s^H of one normalised snapshot, :127), so the
noise-subspace denominator is M - |a^H s|^2 exactly and MUSIC shares beamforming's steering
contraction |A^H S|^2; both run in librsl's MFMA scan kernel (``rsl_doa``).  ESPRIT's SVD of the
(M-1)x2 shift matrix reduces to a 2x2 Hermitian eigenproblem, evaluated in fp64 (``rsl_cell_extras``).
``num_sources != 1`` runs the general subspace forms in fp64 (``rsl_music_subspace`` / ``rsl_esprit_subspace``):
with a rank-1 R the reference's larger signal subspaces contain null-space vectors that LAPACK picks by round-off;
the device fixes them by a Householder completion (see rsl_subspace.hip and tests/test_gpu_dropin.py for which
outputs are reference-determined).
"""
from __future__ import annotations

import logging
from typing import Dict, List, Optional, Tuple

import numpy as np

from rsl import ops, tables
from rsl.runtime import get_context

logger = logging.getLogger(__name__)


class AngleEstimator:
    """ULA angle estimator with the reference's constructor/attributes/methods (angle_estimation.py:23-365)."""

    def __init__(self, fc: float = 77e9, antenna_spacing: float = None, num_antennas: int = 8,
                 search_range: Tuple[float, float] = (-90, 90), search_resolution: float = 0.5):
        self.fc = fc
        self.c = 3e8
        self.lambda_c = self.c / self.fc
        self.antenna_spacing = antenna_spacing or (self.lambda_c / 2)
        self.num_antennas = num_antennas
        self.search_range = search_range
        self.search_resolution = search_resolution
        self.antenna_positions = np.arange(self.num_antennas) * self.antenna_spacing
        self.azimuth_grid = tables.azimuth_grid(search_range, search_resolution)
        self._steer = tables.steering_matrix(self.azimuth_grid, self.antenna_positions, self.lambda_c)
        self._esprit_scale = self.lambda_c / (2 * np.pi * self.antenna_spacing)
        logger.info("Initialized angle estimator:")
        logger.info(f"  Antennas: {self.num_antennas}, spacing: {self.antenna_spacing * 1000:.1f} mm")
        logger.info(f"  Search range: {search_range[0]}° to {search_range[1]}°")
        logger.info(f"  Search resolution: {search_resolution}°")

    # -- a11 / a12 ------------------------------------------------------------------------------------
    def extract_spatial_signature(self, rds: np.ndarray, range_bin: int, doppler_bin: int) -> np.ndarray:
        """rds[:, r, d] normalised to unit power (angle_estimation.py:67-90), gathered on the device."""
        sig, _, _ = ops.cell_extras(rds=rds, rbins=[range_bin], dbins=[doppler_bin], want_sig=True)
        return sig[0]

    def generate_steering_vector(self, azimuth_deg: float) -> np.ndarray:
        """exp(j 2 pi x_m sin(az) / lambda) (angle_estimation.py:92-107), host fp64 table row."""
        return tables.steering_matrix([azimuth_deg], self.antenna_positions, self.lambda_c)[0]

    # -- a13 .. a16 -------------------------------------------------------------------------------------
    def music_spectrum(self, spatial_signature: np.ndarray, num_sources: int = 1) -> np.ndarray:
        """1/|a^H E_n E_n^H a| over the azimuth grid, 0 where <= 1e-12 (angle_estimation.py:109-154)."""
        if num_sources != 1:
            return ops.subspace_music(np.asarray(spatial_signature)[None], self._steer, num_sources)[0]
        _, spec = ops.doa('music', self._steer, sigs=np.asarray(spatial_signature)[None], want_spec=True)
        return spec[0]

    def estimate_angle_music(self, spatial_signature: np.ndarray, num_sources: int = 1) -> Tuple[float, np.ndarray]:
        if num_sources != 1:
            spec = self.music_spectrum(spatial_signature, num_sources)
            return self.azimuth_grid[np.argmax(spec)], spec
        idx, spec = ops.doa('music', self._steer, sigs=np.asarray(spatial_signature)[None], want_spec=True)
        return self.azimuth_grid[idx[0]], spec[0]

    def estimate_angle_esprit(self, spatial_signature: np.ndarray, num_sources: int = 1) -> float:
        """Closed-form rank-1 ESPRIT in fp64 (angle_estimation.py:178-225); 0.0 if it fails, as the reference."""
        if num_sources != 1:
            return float(ops.subspace_esprit(np.asarray(spatial_signature)[None], num_sources,
                                             self._esprit_scale)[0])
        try:
            _, esp, _ = ops.cell_extras(sigs=np.asarray(spatial_signature)[None], esprit_scale=self._esprit_scale,
                                        want_esprit=True)
            return esp[0]
        except (ValueError, RuntimeError) as e:
            logger.warning(f"ESPRIT failed: {e}")
            return 0.0

    def estimate_angle_beamforming(self, spatial_signature: np.ndarray) -> Tuple[float, np.ndarray]:
        idx, spec = ops.doa('beamforming', self._steer, sigs=np.asarray(spatial_signature)[None], want_spec=True)
        return self.azimuth_grid[idx[0]], spec[0]

    # -- a17 ------------------------------------------------------------------------------------------
    def process_targets(self, rds: np.ndarray, peak_info: Dict, method: str = 'music') -> List[Dict]:
        """All peaks in one batched device pass (angle_estimation.py:253-309); same target dicts."""
        peaks = list(peak_info['peaks'])
        if method not in ('music', 'esprit', 'beamforming'):
            for _ in peaks:  # the reference raises inside its per-target try and skips every target
                logger.warning(f"Error processing target: Unknown method: {method}")
            logger.info(f"Processed 0 targets using {method}")
            return []
        A, S, C = rds.shape
        keep = []
        for p in peaks:
            r, d = p['range_bin'], p['doppler_bin']
            if -S <= r < S and -C <= d < C:
                keep.append(p)
            else:
                logger.warning("Error processing target: index out of bounds")
        rb = np.array([p['range_bin'] % S for p in keep], dtype=np.int64)
        db = np.array([p['doppler_bin'] % C for p in keep], dtype=np.int64)
        ctx = get_context()
        d_rds = ops.as_dev_c64(ctx, rds)
        sig, esp, _ = ops.cell_extras(rds=d_rds, rbins=rb, dbins=db, esprit_scale=self._esprit_scale,
                                      want_sig=True, want_esprit=(method == 'esprit'))
        if method == 'esprit':
            angles, spec = esp, None
        else:
            idx, spec = ops.doa(method, self._steer, rds=d_rds, rbins=rb, dbins=db, want_spec=True)
            angles = self.azimuth_grid[idx]
        targets = []
        for n, p in enumerate(keep):
            ang = angles[n]
            targets.append({'range_m': p['range_m'], 'doppler_hz': p['doppler_hz'], 'power_db': p['power_db'],
                            'azimuth_deg': ang, 'azimuth_rad': np.radians(ang), 'antenna': p['antenna'],
                            'range_bin': p['range_bin'], 'doppler_bin': p['doppler_bin'],
                            'spatial_signature': sig[n], 'spectrum': None if spec is None else spec[n]})
        logger.info(f"Processed {len(targets)} targets using {method}")
        return targets

    def process_targets_refined(self, rds: np.ndarray, peak_info: Dict, method: str = 'music',
                                window_type: str = 'hann') -> List[Dict]:
        """process_targets plus the point cloud (ops.refine_cells): every target dict gains 'range_m_refined',
        'doppler_hz_refined', 'azimuth_deg_refined', 'x_m', 'y_m', 'range_offset' and 'doppler_offset', refined below
        the bin and grid spacing from the antenna-summed power around the cell and the beamforming values around the
        scan's argmax.  The labels continue the targets' own axes: one range (Doppler) bin is the spacing of the
        peaks' 'range_m' ('doppler_hz') labels, taken from peak_info['range_bins_m'] / ['doppler_bins_hz'] (the
        axes extract_range_doppler_peaks returns) where given, else the columns count bins.  window_type: the fast-time window the RDS was formed with (it selects the range estimator).
        method 'esprit' has no grid index; its targets are refined around the MUSIC argmax."""
        targets = self.process_targets(rds, peak_info, method)
        if not targets:
            return targets
        A, S, C = rds.shape
        rb = np.array([t['range_bin'] % S for t in targets], dtype=np.int64)
        db = np.array([t['doppler_bin'] % C for t in targets], dtype=np.int64)

        def axis(name, n):  # (origin, step) of a label axis: the peak dictionary's own where it carries one
            ax = peak_info.get(name) if hasattr(peak_info, 'get') else None
            if ax is not None and len(ax) == n and n > 1:
                return float(ax[0]), float(ax[-1] - ax[0]) / (n - 1)
            return 0.0, 1.0
        r0, r_step = axis('range_bins_m', S)
        d0, d_step = axis('doppler_bins_hz', C)
        res = ops.refine_cells(self._steer, self.azimuth_grid, rds=rds, rbins=rb, dbins=db,
                               method='beamforming' if method == 'beamforming' else 'music',
                               range_mode=tables.refine_mode_for_window(window_type), doppler_mode='rect',
                               axes=(r0, r_step, d0, d_step))
        for n, t in enumerate(targets):
            t.update(range_m_refined=float(res['range'][n]), doppler_hz_refined=float(res['doppler'][n]),
                     azimuth_deg_refined=float(res['azimuth_deg'][n]), x_m=float(res['x'][n]), y_m=float(res['y'][n]),
                     range_offset=float(res['range_offset'][n]), doppler_offset=float(res['doppler_offset'][n]))
        return targets

    def register_scans(self, prev_targets: List[Dict], cur_targets: List[Dict], init=None, **params) -> Dict:
        """The rigid motion between two scans of process_targets_refined (ops.register_scans, specified in
        include/rsl.h as rsl_scan_register): the yaw increment and the displacement that map the current targets'
        ('x_m', 'y_m') onto the previous scan's, p' = R(theta) p + t.  A target dict's optional 'weight' (0: a mover)
        is its vote.  init = (theta, t_x, t_y) start values, e.g. (0, v_x dt, v_y dt) from the velocity solve;
        params: h, h_coarse, dtheta, k, iters, shrink, tol, w_min.  Returns dict(theta_rad, theta_deg, t_x, t_y,
        support, rms, peak_ratio, updates, flag); flag 1: too little overlap, the start values are returned."""
        def rows(targets):
            pts = np.zeros((len(targets), 8), np.float32)
            for n, t in enumerate(targets):
                pts[n, 3], pts[n, 4] = t['x_m'], t['y_m']
            return pts, np.array([t.get('weight', 1.0) for t in targets], np.float32)
        (pp, pw), (cp, cw) = rows(prev_targets), rows(cur_targets)
        res = ops.register_scans(cp, np.array([0, len(cp)], np.int64), weight=cw, prev=dict(points=pp, weight=pw),
                                 init=None if init is None else np.asarray(init, np.float64).reshape(1, 3), **params)
        out = {k: float(res[k][0]) for k in ops.REGISTRATION_COLUMNS}
        out['theta_rad'] = out.pop('theta')
        out['theta_deg'] = float(np.degrees(out['theta_rad']))
        out['updates'], out['flag'] = int(out['updates']), int(out['flag'])
        return out

    def process_targets_smoothed(self, rds: np.ndarray, peaks: Dict, num_sources: int = 0, sub_len: Optional[int] = None,
                                 rel: float = 0.05, max_sources: int = 3) -> List[Dict]:
        """process_targets with the forward-backward spatially smoothed MUSIC (ops.doa_smoothed): several angles per
        target.  The dicts of process_targets plus 'angles_deg' (list, deepest null first), 'num_sources' (the model
        order used: num_sources, or with 0 the number of eigenvalues >= rel * the largest, at most max_sources) and
        'eigenvalues' (descending, of the smoothed sub_len x sub_len covariance).  'azimuth_deg' is the first angle
        (NaN when the null spectrum has no local minimum) and 'spectrum' the pseudo-spectrum 1 / den (0 where den <=
        1e-12, the rule of music_spectrum).  A fixed num_sources is the dependable setting: rel depends on the SNR."""
        plist = list(peaks['peaks'])
        A, S, C = rds.shape
        keep = []
        for p in plist:
            r, d = p['range_bin'], p['doppler_bin']
            if -S <= r < S and -C <= d < C:
                keep.append(p)
            else:
                logger.warning("Error processing target: index out of bounds")
        rb = np.array([p['range_bin'] % S for p in keep], dtype=np.int64)
        db = np.array([p['doppler_bin'] % C for p in keep], dtype=np.int64)
        ctx = get_context()
        d_rds = ops.as_dev_c64(ctx, rds)
        sig, _, _ = ops.cell_extras(rds=d_rds, rbins=rb, dbins=db, esprit_scale=self._esprit_scale, want_sig=True)
        res = ops.doa_smoothed(self._steer, rds=d_rds, rbins=rb, dbins=db, sub_len=sub_len, num_sources=num_sources,
                               rel=rel, nmax=max_sources, want_eig=True, want_spec=True, grid_deg=self.azimuth_grid)
        targets = []
        for n, p in enumerate(keep):
            angs = [float(a) for a in res['deg'][n] if not np.isnan(a)]
            ang = angs[0] if angs else float('nan')
            den = res['spec'][n]
            spec = np.zeros_like(den)
            np.divide(1.0, den, out=spec, where=den > 1e-12)
            targets.append({'range_m': p['range_m'], 'doppler_hz': p['doppler_hz'], 'power_db': p['power_db'],
                            'azimuth_deg': ang, 'azimuth_rad': np.radians(ang), 'antenna': p['antenna'],
                            'range_bin': p['range_bin'], 'doppler_bin': p['doppler_bin'],
                            'spatial_signature': sig[n], 'spectrum': spec, 'angles_deg': angs,
                            'num_sources': int(res['nsrc'][n]), 'eigenvalues': res['eig'][n]})
        logger.info(f"Processed {len(targets)} targets using smoothed music")
        return targets

    def range_azimuth_map(self, rds: np.ndarray, method: str = 'capon', doppler: Optional[Tuple[int, int]] = None,
                          loading: float = 1e-2) -> Dict:
        """The range-azimuth power map of an RDS [A, S, C] on this estimator's grid (ops.range_azimuth_map): every
        range bin's spatial covariance over its Doppler bins (doppler = (c0, c1); None: all), then 'bartlett' (a^H R a
        / A^2) or 'capon' (1 / a^H R_l^-1 a, diagonal loading `loading`).  Returns 'map' f64 [S, G], 'angles_deg' (the
        grid) and 'arg' i64 [S] (the grid index of every range bin's maximum)."""
        res = ops.range_azimuth_map(self._steer, rds=rds, method=method, doppler=doppler, loading=loading,
                                    want_arg=True)
        return {'map': res['map'], 'angles_deg': self.azimuth_grid, 'arg': res['arg']}

    def visualize_angle_spectrum(self, targets: List[Dict], save_path: Optional[str] = None) -> None:
        if not targets:
            logger.warning("No targets to visualize")
            return
        import matplotlib.pyplot as plt
        fig, axes = plt.subplots(2, 2, figsize=(12, 10))
        angles = [t['azimuth_deg'] for t in targets]
        ranges = [t['range_m'] for t in targets]
        powers = [t['power_db'] for t in targets]
        axes[0, 0].hist(angles, bins=20, alpha=0.7)
        axes[0, 0].set_title('Angle Distribution')
        axes[0, 1].scatter(angles, ranges, c=powers, cmap='viridis', alpha=0.7)
        axes[0, 1].set_title('Range vs Angle')
        axes[1, 0].scatter(angles, powers, alpha=0.7)
        axes[1, 0].set_title('Power vs Angle')
        if targets[0]['spectrum'] is not None:
            axes[1, 1].plot(self.azimuth_grid, 10 * np.log10(targets[0]['spectrum'] + 1e-12))
            axes[1, 1].set_title('MUSIC Spectrum')
        plt.tight_layout()
        if save_path:
            plt.savefig(save_path, dpi=150, bbox_inches='tight')
        plt.show()


def extract_angles_from_rds(rds_path: str, peak_info_path: str, output_path: str, method: str = 'music',
                            radar_params: Dict = None) -> Dict:
    """File wrapper (angle_estimation.py:368-417)."""
    rds = np.load(rds_path)
    peak_info = dict(np.load(peak_info_path, allow_pickle=True))
    logger.info(f"Loaded RDS: {rds.shape}")
    logger.info(f"Found {len(peak_info['peaks'])} peaks")
    if radar_params is None:
        radar_params = {'fc': 77e9, 'antenna_spacing': 3e8 / (2 * 77e9), 'num_antennas': 8}
    est = AngleEstimator(**radar_params)
    targets = est.process_targets(rds, peak_info, method)
    np.savez(output_path, targets=targets, radar_params=radar_params)
    logger.info(f"Saved angle estimates for {len(targets)} targets")
    return {'num_targets': len(targets), 'method': method, 'targets': targets}


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description='Extract angles from RDS data')
    ap.add_argument('--rds', required=True)
    ap.add_argument('--peaks', required=True)
    ap.add_argument('--out', required=True)
    ap.add_argument('--method', choices=['music', 'esprit', 'beamforming'], default='music')
    a = ap.parse_args()
    print(f"Angle extraction complete: {extract_angles_from_rds(a.rds, a.peaks, a.out, a.method)}")
