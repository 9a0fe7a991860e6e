// tdoa_cgo.go -- the cgo shim a maintainer of KX0U-Jim/tdoa-geolocation adds next to processor.go
// (as tdoa_gpu.go) to route the correlation path through libtdoa_mi355x.so.
//
// SOURCE ONLY: there is no Go toolchain in the build image, so this file is never compiled here.
// It is a pointer + length pass-through with no logic; everything it forwards to is exercised
// through the same C ABI by tests/ (ctypes) and examples/pair_from_c.c (C99).
// Call sites it replaces: processor.go:818, :838 (crossCorrelate), correlation_sanity.go:50,55;
// see INTEGRATION.md section 1 for the full table.
package main

/*
#cgo CFLAGS: -I${SRCDIR}/tdoa-mi355x/include
#cgo LDFLAGS: -L${SRCDIR}/tdoa-mi355x/tdoa-geolocation_amd -ltdoa_mi355x -Wl,-rpath,${SRCDIR}/tdoa-mi355x/tdoa-geolocation_amd
#include <stdlib.h>
#include "tdoa_mi355x.h"
*/
import "C"

import (
	"fmt"
	"unsafe"
)

// gpuCorrelator owns one tdoa_ctx (one GPU). Not safe for concurrent use (the reference is single-goroutine).
type gpuCorrelator struct{ ctx *C.tdoa_ctx }

// goLagSet: search the lags timeDomainCorrelation searches (processor.go:650-678: shorter input = template, lags
// [0, max(1, min(maxLag, Ls-Lt))), first strict maximum) instead of the signed range -maxLag < lag < maxLag.
func newGPUCorrelator(device int, goLagSet bool) (*gpuCorrelator, error) {
	var p C.tdoa_params
	C.tdoa_default_params(&p) // 2e6 Hz, maxLag 20000, block 1000, gate 0.001, window 2 000 000
	p.device = C.int32_t(device)
	if goLagSet {
		p.lag_mode = C.TDOA_LAGS_GO
	}
	var ctx *C.tdoa_ctx
	if rc := C.tdoa_create(&p, &ctx); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_create: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	return &gpuCorrelator{ctx: ctx}, nil
}

func (g *gpuCorrelator) Close() { C.tdoa_destroy(g.ctx) }

func c64ptr(s []complex64) *C.float {
	if len(s) == 0 {
		return nil
	}
	return (*C.float)(unsafe.Pointer(&s[0])) // Go complex64 == {float32 re, float32 im}
}

// crossCorrelate is the drop-in for (*TDOAProcessor).crossCorrelate (processor.go:619).
func (g *gpuCorrelator) crossCorrelate(signal1, signal2 []complex64) (int, float64) {
	var delay C.int32_t
	var corr C.double
	rc := C.tdoa_cross_correlate_c64(g.ctx, c64ptr(signal1), C.size_t(len(signal1)),
		c64ptr(signal2), C.size_t(len(signal2)), &delay, &corr)
	if rc != C.TDOA_OK {
		panic(fmt.Sprintf("tdoa_cross_correlate_c64: %s (%s)", C.GoString(C.tdoa_strerror(rc)),
			C.GoString(C.tdoa_last_error(g.ctx))))
	}
	return int(delay), float64(corr)
}

// processCaptures is the batched path: raw .dat bytes of every station in, one peak per
// (window, pair) out, pairs ordered i<j like processor.go:816-817.
func (g *gpuCorrelator) processCaptures(dat [][]byte) ([]C.tdoa_peak, int, error) {
	for s, b := range dat {
		if len(b) < 2 { // &b[0] of an empty slice panics; an empty capture cannot be windowed anyway
			return nil, 0, fmt.Errorf("upload %d: capture is empty", s)
		}
		rc := C.tdoa_capture_upload(g.ctx, C.int(s), (*C.uint8_t)(unsafe.Pointer(&b[0])), C.size_t(len(b)/2))
		if rc != C.TDOA_OK {
			return nil, 0, fmt.Errorf("upload %d: %s", s, C.GoString(C.tdoa_last_error(g.ctx)))
		}
	}
	var perBlock, total C.int
	C.tdoa_num_windows(g.ctx, &perBlock, &total)
	pairs := int(C.tdoa_num_pairs(g.ctx))
	out := make([]C.tdoa_peak, int(total)*pairs)
	if rc := C.tdoa_process(g.ctx, 0, 1, &out[0], nil); rc != C.TDOA_OK {
		return nil, 0, fmt.Errorf("tdoa_process: %s", C.GoString(C.tdoa_last_error(g.ctx)))
	}
	return out, pairs, nil
}

// processCapturesFine adds the sub-sample delay and the |TDOA| gate (in samples) to every peak.
func (g *gpuCorrelator) processCapturesFine(gate float64) ([]C.tdoa_peak, []C.tdoa_fine_peak, error) {
	var perBlock, total C.int
	C.tdoa_num_windows(g.ctx, &perBlock, &total)
	n := int(total) * int(C.tdoa_num_pairs(g.ctx))
	peaks, fine := make([]C.tdoa_peak, n), make([]C.tdoa_fine_peak, n)
	if rc := C.tdoa_process_fine(g.ctx, 0, 1, C.double(gate), &peaks[0], &fine[0]); rc != C.TDOA_OK {
		return nil, nil, fmt.Errorf("tdoa_process_fine: %s", C.GoString(C.tdoa_last_error(g.ctx)))
	}
	return peaks, fine, nil
}

// ProcessPeaks returns the k strongest separate peaks of every (window, pair) correlation, strongest first, and how many
// each holds: peak 1 is processCaptures' peak; the others are local maxima more than minSeparation lags from every peak
// already chosen (multipath, a second emitter, the main-to-sidelobe ratio).
func (g *gpuCorrelator) ProcessPeaks(k, minSeparation int) ([]C.tdoa_peak, []C.int32_t, error) {
	var perBlock, total C.int
	C.tdoa_num_windows(g.ctx, &perBlock, &total)
	n := int(total) * int(C.tdoa_num_pairs(g.ctx))
	if n == 0 || k < 1 {
		return nil, nil, fmt.Errorf("tdoa_process_peaks: no pair-windows or k < 1")
	}
	peaks, count := make([]C.tdoa_peak, n*k), make([]C.int32_t, n)
	if rc := C.tdoa_process_peaks(g.ctx, 0, 1, C.int(k), C.int(minSeparation), &peaks[0], &count[0]); rc != C.TDOA_OK {
		return nil, nil, fmt.Errorf("tdoa_process_peaks: %s", C.GoString(C.tdoa_last_error(g.ctx)))
	}
	return peaks, count, nil
}

// ProcessStacked adds the correlation surfaces of windowsPerStack consecutive windows of a block (0: the whole block) lag by
// lag and returns, per stack and pair, up to k peaks, their count and peak 1 refined to a fraction of a sample: one delay
// per station pair and frequency block where single windows are too noisy for their own argmax (processor.go:770-782).
func (g *gpuCorrelator) ProcessStacked(windowsPerStack, k, minSeparation int, gate float64) ([]C.tdoa_peak, []C.int32_t, []C.tdoa_fine_peak, error) {
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(g.ctx, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, nil, nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	n := int(total) * int(C.tdoa_num_pairs(g.ctx))
	if n == 0 || k < 1 {
		return nil, nil, nil, fmt.Errorf("tdoa_process_stacked: no stack-pairs or k < 1")
	}
	peaks, count, fine := make([]C.tdoa_peak, n*k), make([]C.int32_t, n), make([]C.tdoa_fine_peak, n)
	if rc := C.tdoa_process_stacked(g.ctx, 0, 1, C.int(windowsPerStack), C.int(k), C.int(minSeparation), C.double(gate),
		&peaks[0], &count[0], &fine[0], nil, nil); rc != C.TDOA_OK {
		return nil, nil, nil, fmt.Errorf("tdoa_process_stacked: %s", C.GoString(C.tdoa_last_error(g.ctx)))
	}
	return peaks, count, fine, nil
}

// ProcessStackedDrift is ProcessStacked along the best of the 2*maxDrift+1 lag slopes h/driftDen lags per window, searched
// per stack and pair: shift(h, j) = sgn(h)*((2|h|j + D) div (2D)) lags for window j of a stack, terms outside the searched
// range contributing 0.  drift holds h* per stack-pair (the pair's relative clock rate is h*/(driftDen*window_len)), the
// other results are those of the stack taken along that slope; the reported lag is the lag at the stack's first window.
// One context sums all its windows: there is no group form of this call.
func (g *gpuCorrelator) ProcessStackedDrift(windowsPerStack, k, minSeparation int, gate float64, maxDrift, driftDen int) ([]C.tdoa_peak, []C.int32_t, []C.tdoa_fine_peak, []C.int32_t, error) {
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(g.ctx, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, nil, nil, nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	n := int(total) * int(C.tdoa_num_pairs(g.ctx))
	if n == 0 || k < 1 {
		return nil, nil, nil, nil, fmt.Errorf("tdoa_process_stacked_drift: no stack-pairs or k < 1")
	}
	peaks, count, fine, drift := make([]C.tdoa_peak, n*k), make([]C.int32_t, n), make([]C.tdoa_fine_peak, n), make([]C.int32_t, n)
	if rc := C.tdoa_process_stacked_drift(g.ctx, C.int(windowsPerStack), C.int(k), C.int(minSeparation), C.double(gate),
		C.int(maxDrift), C.int(driftDen), &peaks[0], &count[0], &fine[0], nil, nil, &drift[0], nil); rc != C.TDOA_OK {
		return nil, nil, nil, nil, fmt.Errorf("tdoa_process_stacked_drift: %s", C.GoString(C.tdoa_last_error(g.ctx)))
	}
	return peaks, count, fine, drift, nil
}

// ProcessTrack is the best delay track through every stack's windows: one lag per window, consecutive lags at most maxStep
// apart, the sum of the windows' fixed-point correlation values along the track the largest (the header's "delay tracks").
// score holds one record per stack-pair (lag: the track's lag at the stack's first window, corr: the signed sum along the
// track on C's scale), lags and values stackLen entries per stack-pair (positions past a shorter stack's end are 0).
// A track crosses every window of its stack: there is no group form of this call.
func (g *gpuCorrelator) ProcessTrack(windowsPerStack, maxStep int) (score []C.tdoa_peak, lags []C.int32_t, values []C.double, stackLen int, err error) {
	var perBlock, total, wpb C.int
	if rc := C.tdoa_num_stacks(g.ctx, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, nil, nil, 0, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	if rc := C.tdoa_num_windows(g.ctx, &wpb, nil); rc != C.TDOA_OK {
		return nil, nil, nil, 0, fmt.Errorf("tdoa_num_windows: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	stackLen = int(wpb)
	if windowsPerStack > 0 && windowsPerStack < stackLen {
		stackLen = windowsPerStack
	}
	n := int(total) * int(C.tdoa_num_pairs(g.ctx))
	if n == 0 || stackLen == 0 {
		return nil, nil, nil, 0, fmt.Errorf("tdoa_process_track: no stack-pairs")
	}
	score, lags, values = make([]C.tdoa_peak, n), make([]C.int32_t, n*stackLen), make([]C.double, n*stackLen)
	if rc := C.tdoa_process_track(g.ctx, C.int(windowsPerStack), C.int(maxStep), &score[0], &lags[0], &values[0], nil, nil); rc != C.TDOA_OK {
		return nil, nil, nil, 0, fmt.Errorf("tdoa_process_track: %s", C.GoString(C.tdoa_last_error(g.ctx)))
	}
	return score, lags, values, stackLen, nil
}

// centrePtr is the centres as the C ABI takes them: nil (all 0), or one int32 per station.
func centrePtr(centre []int32) *C.int32_t {
	if len(centre) == 0 {
		return nil
	}
	return (*C.int32_t)(unsafe.Pointer(&centre[0]))
}

// ProcessClosure is the closure search: per stack and station triple i < j < k the three lags that close
// (lag_ij + lag_jk = lag_ik) with the largest summed magnitude within gate lags of the pairs' centres (the header's
// "closure search"), next to what the three independent argmaxes give (own_q, residual) and the runner-up.  centre: one
// lag per station (nil: all 0).  The records are [stack][triple], triples the second return value.
func (g *gpuCorrelator) ProcessClosure(windowsPerStack, gate, minSeparation int, centre []int32) ([]C.tdoa_closure, int, error) {
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(g.ctx, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, 0, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	triples := int(C.tdoa_num_triples(g.ctx))
	if int(total)*triples == 0 {
		return nil, 0, fmt.Errorf("tdoa_process_closure: no stacks or fewer than three stations")
	}
	out := make([]C.tdoa_closure, int(total)*triples)
	if rc := C.tdoa_process_closure(g.ctx, C.int(windowsPerStack), C.int(gate), C.int(minSeparation), centrePtr(centre), &out[0]); rc != C.TDOA_OK {
		return nil, 0, fmt.Errorf("tdoa_process_closure: %s", C.GoString(C.tdoa_last_error(g.ctx)))
	}
	return out, triples, nil
}

// tablePtr is a delay table as the C ABI takes it: nil (forget the table), or nCells * nStations int32.
func tablePtr(delay []int32) *C.int32_t {
	if len(delay) == 0 {
		return nil
	}
	return (*C.int32_t)(unsafe.Pointer(&delay[0]))
}

// LocateGridTable is the host-only table of a latitude / longitude grid (the header's "delay-table search"): cell
// r*cols + c at (lat0 + r*dlat, lon0 + c*dlon, heightM), one delay per station in units of 1/16 sample.  stationsLLE holds
// latitude, longitude and elevation per station.
func LocateGridTable(stationsLLE []float64, lat0, lon0, dlat, dlon float64, rows, cols int, heightM, sampleRate float64) ([]int32, error) {
	n := len(stationsLLE) / 3
	if n < 1 || rows < 1 || cols < 1 || rows*cols > 1<<22 {
		return nil, fmt.Errorf("tdoa_locate_grid_table: no stations, or rows*cols outside 1 .. 2^22")
	}
	delay := make([]int32, rows*cols*n)
	if rc := C.tdoa_locate_grid_table((*C.double)(unsafe.Pointer(&stationsLLE[0])), C.int(n), C.double(lat0), C.double(lon0),
		C.double(dlat), C.double(dlon), C.int(rows), C.int(cols), C.double(heightM), C.double(sampleRate),
		(*C.int32_t)(unsafe.Pointer(&delay[0]))); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_locate_grid_table: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	return delay, nil
}

// LocateSetTable hands the context its delay table [nCells][nStations] (nil: forget it); nCols gives cells their rows and
// columns.  The table stays on the device until it is replaced.
func (g *gpuCorrelator) LocateSetTable(delay []int32, nCells, nCols, nStations int) error {
	if rc := C.tdoa_locate_set_table(g.ctx, tablePtr(delay), C.int(nCells), C.int(nCols), C.int(nStations)); rc != C.TDOA_OK {
		return fmt.Errorf("tdoa_locate_set_table: %s", C.GoString(C.tdoa_last_error(g.ctx)))
	}
	return nil
}

// ProcessLocate is the delay-table search: per stack the table's cell with the largest summed magnitude of all pairs' stacks
// at the cell's lags, the runner-up, and per pair the lag and the signed correlation at the best cell ([stack][pair]; what
// tdoa_solve_surface takes as range differences and weights).
func (g *gpuCorrelator) ProcessLocate(windowsPerStack, minSeparation int) (loc []C.tdoa_location, lags []int32, corr []float64, err error) {
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(g.ctx, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, nil, nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	pairs := int(C.tdoa_num_pairs(g.ctx))
	if int(total)*pairs == 0 {
		return nil, nil, nil, fmt.Errorf("tdoa_process_locate: no stacks or fewer than two stations")
	}
	loc = make([]C.tdoa_location, int(total))
	lags = make([]int32, int(total)*pairs)
	corr = make([]float64, int(total)*pairs)
	if rc := C.tdoa_process_locate(g.ctx, C.int(windowsPerStack), C.int(minSeparation), &loc[0], (*C.int32_t)(unsafe.Pointer(&lags[0])),
		(*C.double)(unsafe.Pointer(&corr[0])), nil); rc != C.TDOA_OK {
		return nil, nil, nil, fmt.Errorf("tdoa_process_locate: %s", C.GoString(C.tdoa_last_error(g.ctx)))
	}
	return loc, lags, corr, nil
}

// ProcessLocateMulti finds up to nEmitters emitters per stack (the header's "several emitters per stack"): round 0 is
// ProcessLocate's search, every later round searches again with the lags within guard of the earlier rounds' cells' lags
// counting 0 in every pair.  loc is [round][stack], lags and corr [round][stack][pair]; an excluded pair reports its lag and
// 0.0, so tdoa_solve_surface gives it no weight.
func (g *gpuCorrelator) ProcessLocateMulti(windowsPerStack, nEmitters, guard, minSeparation int) (loc []C.tdoa_location, lags []int32, corr []float64, err error) {
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(g.ctx, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, nil, nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	pairs := int(C.tdoa_num_pairs(g.ctx))
	if int(total)*pairs == 0 || nEmitters < 1 {
		return nil, nil, nil, fmt.Errorf("tdoa_process_locate_multi: no stacks, fewer than two stations or no rounds")
	}
	loc = make([]C.tdoa_location, nEmitters*int(total))
	lags = make([]int32, nEmitters*int(total)*pairs)
	corr = make([]float64, nEmitters*int(total)*pairs)
	if rc := C.tdoa_process_locate_multi(g.ctx, C.int(windowsPerStack), C.int(nEmitters), C.int(guard), C.int(minSeparation), &loc[0],
		(*C.int32_t)(unsafe.Pointer(&lags[0])), (*C.double)(unsafe.Pointer(&corr[0])), nil); rc != C.TDOA_OK {
		return nil, nil, nil, fmt.Errorf("tdoa_process_locate_multi: %s", C.GoString(C.tdoa_last_error(g.ctx)))
	}
	return loc, lags, corr, nil
}

// ProcessLocateTrack follows an emitter through the stacks of every block on the delay-table search's maps (the header's
// "cell tracks"): per block one cell per stack, consecutive cells at most maxStep rows and columns apart, with the largest
// summed score, and the runner-up.  cells and own are [block][stacks per block] (the track's cell in every stack and that
// stack's own score there), lags and corr [stack][pair] at the track's cell, each row what tdoa_solve_surface takes.
func (g *gpuCorrelator) ProcessLocateTrack(windowsPerStack, maxStep, minSeparation int) (track []C.tdoa_cell_track, cells []int32, own []int64, lags []int32, corr []float64, err error) {
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(g.ctx, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, nil, nil, nil, nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	pairs := int(C.tdoa_num_pairs(g.ctx))
	if int(total)*pairs == 0 {
		return nil, nil, nil, nil, nil, fmt.Errorf("tdoa_process_locate_track: no stacks or fewer than two stations")
	}
	track = make([]C.tdoa_cell_track, int(total)/int(perBlock))
	cells = make([]int32, int(total))
	own = make([]int64, int(total))
	lags = make([]int32, int(total)*pairs)
	corr = make([]float64, int(total)*pairs)
	if rc := C.tdoa_process_locate_track(g.ctx, C.int(windowsPerStack), C.int(maxStep), C.int(minSeparation), &track[0],
		(*C.int32_t)(unsafe.Pointer(&cells[0])), (*C.int64_t)(unsafe.Pointer(&own[0])), (*C.int32_t)(unsafe.Pointer(&lags[0])),
		(*C.double)(unsafe.Pointer(&corr[0])), nil); rc != C.TDOA_OK {
		return nil, nil, nil, nil, nil, fmt.Errorf("tdoa_process_locate_track: %s", C.GoString(C.tdoa_last_error(g.ctx)))
	}
	return track, cells, own, lags, corr, nil
}

// TrackRounds holds what ProcessLocateTrackMulti returns, every slice with the round as its first index: Track
// [round][block], Cells and Own [round][block][stacks per block], Pairs [round][stack][2] (pairs_in, reserved), Lags and Corr
// [round][stack][pair].
type TrackRounds struct {
	Track []C.tdoa_cell_track
	Cells []int32
	Own   []int64
	Pairs []int32
	Lags  []int32
	Corr  []float64
}

func newTrackRounds(nEmitters, total, perBlock, pairs int) *TrackRounds {
	return &TrackRounds{
		Track: make([]C.tdoa_cell_track, nEmitters*(total/perBlock)),
		Cells: make([]int32, nEmitters*total),
		Own:   make([]int64, nEmitters*total),
		Pairs: make([]int32, nEmitters*total*2),
		Lags:  make([]int32, nEmitters*total*pairs),
		Corr:  make([]float64, nEmitters*total*pairs),
	}
}

// ProcessLocateTrackMulti finds up to nEmitters emitters per block as cell tracks (the header's "several emitters per
// block"): round 0 is ProcessLocateTrack's track, every later round tracks again with the lags within guard of the earlier
// rounds' tracks' lags counting 0 in every stack's pairs.  An excluded pair reports its lag and 0.0, so tdoa_solve_surface
// gives it no weight.
func (g *gpuCorrelator) ProcessLocateTrackMulti(windowsPerStack, maxStep, nEmitters, guard, minSeparation int) (*TrackRounds, error) {
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(g.ctx, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	pairs := int(C.tdoa_num_pairs(g.ctx))
	if int(total)*pairs == 0 || nEmitters < 1 {
		return nil, fmt.Errorf("tdoa_process_locate_track_multi: no stacks, fewer than two stations or no rounds")
	}
	r := newTrackRounds(nEmitters, int(total), int(perBlock), pairs)
	if rc := C.tdoa_process_locate_track_multi(g.ctx, C.int(windowsPerStack), C.int(maxStep), C.int(nEmitters), C.int(guard),
		C.int(minSeparation), &r.Track[0], (*C.int32_t)(unsafe.Pointer(&r.Cells[0])), (*C.int64_t)(unsafe.Pointer(&r.Own[0])),
		(*C.int32_t)(unsafe.Pointer(&r.Pairs[0])), (*C.int32_t)(unsafe.Pointer(&r.Lags[0])), (*C.double)(unsafe.Pointer(&r.Corr[0])),
		nil); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_process_locate_track_multi: %s", C.GoString(C.tdoa_last_error(g.ctx)))
	}
	return r, nil
}

// LocateSetClock hands the context the stations' clocks for the delay-table search, [nStacks][nStations] in units of 1/16
// sample (nil: forget them): stack sid's lags are taken from (t[c][j] - t[c][i]) + (clock[sid][j] - clock[sid][i]).  One row per
// stack of the searches that follow; ProcessSync's clocks times 16, or 8*(before + after) for the block between two
// reference blocks.
func (g *gpuCorrelator) LocateSetClock(clock []int32, nStacks, nStations int) error {
	if rc := C.tdoa_locate_set_clock(g.ctx, tablePtr(clock), C.int(nStacks), C.int(nStations)); rc != C.TDOA_OK {
		return fmt.Errorf("tdoa_locate_set_clock: %s", C.GoString(C.tdoa_last_error(g.ctx)))
	}
	return nil
}

// LocateSetStats switches the map statistics on (the header's "map statistics"): while set, ProcessLocate, ProcessLocateMulti,
// ProcessLocateTrack and ProcessLocateTrackMulti also compute one tdoa_map_stats per judged plane -- the live cells' exact
// words at ranks[i] / 65535 of them (32768: the median) and, with foot > 0, the cells that reach foot / 65536 of the way from
// the first of those words to the best.  Up to eight ranks; nil or none: off.  LocateLastStats returns the last call's.
func (g *gpuCorrelator) LocateSetStats(ranks []uint16, foot int) error {
	var p *C.uint16_t
	if len(ranks) > 0 {
		p = (*C.uint16_t)(unsafe.Pointer(&ranks[0]))
	}
	if rc := C.tdoa_locate_set_stats(g.ctx, p, C.int(len(ranks)), C.int(foot)); rc != C.TDOA_OK {
		return fmt.Errorf("tdoa_locate_set_stats: %s", C.GoString(C.tdoa_last_error(g.ctx)))
	}
	return nil
}

// LocateLastStats returns the statistics of the last call of the delay-table family, one per judged plane in the records'
// order ([round][stack] for the searches, [round][track] for the tracks); an error when that call computed none.
func (g *gpuCorrelator) LocateLastStats() ([]C.tdoa_map_stats, error) {
	var n C.int
	C.tdoa_locate_last_stats(g.ctx, nil, 0, &n)
	out := make([]C.tdoa_map_stats, int(n)+1)
	if rc := C.tdoa_locate_last_stats(g.ctx, &out[0], n, &n); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_locate_last_stats: %s", C.GoString(C.tdoa_last_error(g.ctx)))
	}
	return out[:int(n)], nil
}

// LocateSetUpsample sets the lag grid of the delay-table family (the header's "sub-sample locate"): while u in {2, 4, 8, 16} is
// set, ProcessLocate, ProcessLocateMulti, ProcessLocateTrack and ProcessLocateTrackMulti score their cells on the surfaces
// upsampled to 1/u sample, and the lags they return are in units of 1/u sample: a range difference is
// lag / (u * sampleRate) * c.  1: off, the default.
func (g *gpuCorrelator) LocateSetUpsample(u int) error {
	if rc := C.tdoa_locate_set_upsample(g.ctx, C.int(u)); rc != C.TDOA_OK {
		return fmt.Errorf("tdoa_locate_set_upsample: %s", C.GoString(C.tdoa_last_error(g.ctx)))
	}
	return nil
}

// LocateSetFineTable hands the context the zoom locate's second table [nCells][nStations] (nil: forget it): the whole area at z
// fine cells per cell of the table, in nCols columns.  It stays on the device until it is replaced.
func (g *gpuCorrelator) LocateSetFineTable(delay []int32, nCells, nCols, nStations int) error {
	if rc := C.tdoa_locate_set_fine_table(g.ctx, tablePtr(delay), C.int(nCells), C.int(nCols), C.int(nStations)); rc != C.TDOA_OK {
		return fmt.Errorf("tdoa_locate_set_fine_table: %s", C.GoString(C.tdoa_last_error(g.ctx)))
	}
	return nil
}

// LocateZoom is what ProcessLocateZoom returns: the coarse stage's outputs exactly as ProcessLocate's (Loc, Lags, Corr), and per
// stack the zoom's record, its cell's lags (1/u sample with LocateSetUpsample) and signed correlations [stack][pair].
type LocateZoom struct {
	Loc   []C.tdoa_location
	Lags  []int32
	Corr  []float64
	Zoom  []C.tdoa_zoom
	ZLags []int32
	ZCorr []float64
}

func newLocateZoom(stacks, pairs int) *LocateZoom {
	return &LocateZoom{Loc: make([]C.tdoa_location, stacks), Lags: make([]int32, stacks*pairs), Corr: make([]float64, stacks*pairs),
		Zoom: make([]C.tdoa_zoom, stacks), ZLags: make([]int32, stacks*pairs), ZCorr: make([]float64, stacks*pairs)}
}

// ProcessLocateZoom is the zoom locate (the header's "zoom locate"): ProcessLocate's search, then per stack the best of the
// (2h+1)^2 cells of the fine table around z x the stack's best cell, in the same step.  A fine cell's position is the caller's:
// row = Zoom[s].cell / nCols of the fine table, col = the remainder.
func (g *gpuCorrelator) ProcessLocateZoom(windowsPerStack, minSeparation, z, h, fineSeparation int) (*LocateZoom, error) {
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(g.ctx, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	pairs := int(C.tdoa_num_pairs(g.ctx))
	if int(total)*pairs == 0 {
		return nil, fmt.Errorf("tdoa_process_locate_zoom: no stacks or fewer than two stations")
	}
	o := newLocateZoom(int(total), pairs)
	if rc := C.tdoa_process_locate_zoom(g.ctx, C.int(windowsPerStack), C.int(minSeparation), C.int(z), C.int(h), C.int(fineSeparation),
		&o.Loc[0], (*C.int32_t)(unsafe.Pointer(&o.Lags[0])), (*C.double)(unsafe.Pointer(&o.Corr[0])), nil,
		&o.Zoom[0], (*C.int32_t)(unsafe.Pointer(&o.ZLags[0])), (*C.double)(unsafe.Pointer(&o.ZCorr[0])), nil); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_process_locate_zoom: %s", C.GoString(C.tdoa_last_error(g.ctx)))
	}
	return o, nil
}

// LocateMultiZoom is what ProcessLocateMultiZoom returns, every slice [round][stack][...]: the rounds' outputs exactly as
// ProcessLocateMulti's (Loc, Lags, Corr), and per round and stack the zoom's record, its counts (pairs inside the range and
// not excluded at the fine cell, pairs excluded there), its cell's lags (1/u sample with LocateSetUpsample) and signed
// correlations, 0.0 for an excluded pair.
type LocateMultiZoom struct {
	Loc    []C.tdoa_location
	Lags   []int32
	Corr   []float64
	Zoom   []C.tdoa_zoom
	ZPairs []int32
	ZLags  []int32
	ZCorr  []float64
}

func newLocateMultiZoom(rounds, stacks, pairs int) *LocateMultiZoom {
	n := rounds * stacks
	return &LocateMultiZoom{Loc: make([]C.tdoa_location, n), Lags: make([]int32, n*pairs), Corr: make([]float64, n*pairs),
		Zoom: make([]C.tdoa_zoom, n), ZPairs: make([]int32, 2*n), ZLags: make([]int32, n*pairs), ZCorr: make([]float64, n*pairs)}
}

// ProcessLocateMultiZoom is the header's "zoomed rounds": ProcessLocateMulti's rounds, then per round and stack the best of the
// (2h+1)^2 cells of the fine table around z x that round's coarse cell under the mask the round ran under, in the same step.
func (g *gpuCorrelator) ProcessLocateMultiZoom(windowsPerStack, nEmitters, guard, minSeparation, z, h, fineSeparation int) (*LocateMultiZoom, error) {
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(g.ctx, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	pairs := int(C.tdoa_num_pairs(g.ctx))
	if int(total)*pairs == 0 || nEmitters < 1 || nEmitters > 8 {
		return nil, fmt.Errorf("tdoa_process_locate_multi_zoom: no stacks, fewer than two stations or nEmitters outside 1 .. 8")
	}
	o := newLocateMultiZoom(nEmitters, int(total), pairs)
	if rc := C.tdoa_process_locate_multi_zoom(g.ctx, C.int(windowsPerStack), C.int(nEmitters), C.int(guard), C.int(minSeparation), C.int(z),
		C.int(h), C.int(fineSeparation), &o.Loc[0], (*C.int32_t)(unsafe.Pointer(&o.Lags[0])), (*C.double)(unsafe.Pointer(&o.Corr[0])), nil,
		&o.Zoom[0], (*C.int32_t)(unsafe.Pointer(&o.ZPairs[0])), (*C.int32_t)(unsafe.Pointer(&o.ZLags[0])),
		(*C.double)(unsafe.Pointer(&o.ZCorr[0])), nil); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_process_locate_multi_zoom: %s", C.GoString(C.tdoa_last_error(g.ctx)))
	}
	return o, nil
}

// LocateUpsampleTaps returns the u phases' 16 taps at scale 2^15 (host only): the committed table the upsampler uses.
func LocateUpsampleTaps(u int) ([]int32, error) {
	if u < 1 || u > 16 {
		return nil, fmt.Errorf("tdoa_locate_upsample_taps: u must be one of 1, 2, 4, 8, 16")
	}
	taps := make([]int32, u*16)
	if rc := C.tdoa_locate_upsample_taps(C.int(u), (*C.int32_t)(unsafe.Pointer(&taps[0]))); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_locate_upsample_taps: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	return taps, nil
}

// ProcessSync is the clock search (the header's "clock search"): per stack the stations' clocks k_s = centre[s] + x_s,
// |x_s| <= gate, station 0 the gauge, that make all pairs' stacks largest at the lags the known emitter's delays refDelay
// (one per station, units of 1/16 sample) predict -- a joint start, the placing and `rounds` sweeps.  clock is
// [stack][station] in samples, lags and corr [stack][pair].  The caller reads the stacks of the block whose emitter it
// described.
func (g *gpuCorrelator) ProcessSync(windowsPerStack, gate, rounds int, refDelay, centre []int32) (sync []C.tdoa_sync, clock, lags []int32, corr []float64, err error) {
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(g.ctx, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, nil, nil, nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	pairs, stations := int(C.tdoa_num_pairs(g.ctx)), len(refDelay)
	if int(total)*pairs == 0 || stations*(stations-1)/2 != pairs {
		return nil, nil, nil, nil, fmt.Errorf("tdoa_process_sync: no stacks, fewer than two stations, or not one delay per station")
	}
	sync = make([]C.tdoa_sync, int(total))
	clock = make([]int32, int(total)*stations)
	lags = make([]int32, int(total)*pairs)
	corr = make([]float64, int(total)*pairs)
	if rc := C.tdoa_process_sync(g.ctx, C.int(windowsPerStack), C.int(gate), C.int(rounds), tablePtr(refDelay), centrePtr(centre), &sync[0],
		(*C.int32_t)(unsafe.Pointer(&clock[0])), (*C.int32_t)(unsafe.Pointer(&lags[0])), (*C.double)(unsafe.Pointer(&corr[0]))); rc != C.TDOA_OK {
		return nil, nil, nil, nil, fmt.Errorf("tdoa_process_sync: %s", C.GoString(C.tdoa_last_error(g.ctx)))
	}
	return sync, clock, lags, corr, nil
}

// SyncFine is what ProcessSyncFine returns: the coarse stage's outputs exactly as ProcessSync's (Sync, Clock in samples, Lags,
// Corr) and the refinement's: one more record per stack, Clock16 [stack][station] in units of 1/16 sample (what LocateSetClock
// takes), FineLags [stack][pair] in units of 1/U sample and FineCorr, the signed value of the upsampled word there.
type SyncFine struct {
	Sync, Fine  []C.tdoa_sync
	Clock, Lags []int32
	Corr        []float64
	Clock16     []int32
	FineLags    []int32
	FineCorr    []float64
}

func newSyncFine(total, stations, pairs int) *SyncFine {
	return &SyncFine{Sync: make([]C.tdoa_sync, total), Fine: make([]C.tdoa_sync, total), Clock: make([]int32, total*stations),
		Lags: make([]int32, total*pairs), Corr: make([]float64, total*pairs), Clock16: make([]int32, total*stations),
		FineLags: make([]int32, total*pairs), FineCorr: make([]float64, total*pairs)}
}

// ProcessSyncFine is the fine clock search (the header's "fine clock search"): ProcessSync's whole-lag search, then fineRounds
// sweeps that move every station's clock by up to u fine lags of 1/u sample (u one of 2, 4, 8, 16) on the words of the
// surfaces upsampled as LocateSetUpsample defines them, evaluated from Q without materialising them.
func (g *gpuCorrelator) ProcessSyncFine(windowsPerStack, gate, rounds, u, fineRounds int, refDelay, centre []int32) (*SyncFine, error) {
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(g.ctx, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	pairs, stations := int(C.tdoa_num_pairs(g.ctx)), len(refDelay)
	if int(total)*pairs == 0 || stations*(stations-1)/2 != pairs {
		return nil, fmt.Errorf("tdoa_process_sync_fine: no stacks, fewer than two stations, or not one delay per station")
	}
	o := newSyncFine(int(total), stations, pairs)
	if rc := C.tdoa_process_sync_fine(g.ctx, C.int(windowsPerStack), C.int(gate), C.int(rounds), C.int(u), C.int(fineRounds), tablePtr(refDelay),
		centrePtr(centre), &o.Sync[0], (*C.int32_t)(unsafe.Pointer(&o.Clock[0])), (*C.int32_t)(unsafe.Pointer(&o.Lags[0])),
		(*C.double)(unsafe.Pointer(&o.Corr[0])), &o.Fine[0], (*C.int32_t)(unsafe.Pointer(&o.Clock16[0])),
		(*C.int32_t)(unsafe.Pointer(&o.FineLags[0])), (*C.double)(unsafe.Pointer(&o.FineCorr[0]))); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_process_sync_fine: %s", C.GoString(C.tdoa_last_error(g.ctx)))
	}
	return o, nil
}

// SyncLines is what ProcessSyncDrift returns: one record, the clocks (samples) and the rates per block ([3][station]); per
// stack the clock rows in units of 1/16 sample ([stack][station], what LocateSetClock takes for that block) and per stack and
// pair the lag along the line and the signed correlation of that stack there.
type SyncLines struct {
	Line        []C.tdoa_sync_line
	Clock, Rate []int32
	Rows, Lags  []int32
	Corr        []float64
}

func newSyncLines(total, stations, pairs int) *SyncLines {
	return &SyncLines{Line: make([]C.tdoa_sync_line, 3), Clock: make([]int32, 3*stations), Rate: make([]int32, 3*stations),
		Rows: make([]int32, total*stations), Lags: make([]int32, total*pairs), Corr: make([]float64, total*pairs)}
}

func i32Ptr(a []int32) *C.int32_t { return (*C.int32_t)(unsafe.Pointer(&a[0])) }

// ProcessSyncDrift is the clock-line search (the header's "clock lines"): per block the stations' clocks k_s(j) = k_s +
// shift(h_s, j) along the block's stacks, |k_s - centre[s]| <= gate, |h_s| <= maxDrift in units of 1/driftDen lag per stack,
// station 0 the gauge, that make all pairs' signed sums along the block largest at the lags the known emitter's delays
// refDelay predict -- the placing and `rounds` sweeps.  SyncLineClock continues a line past its block.
func (g *gpuCorrelator) ProcessSyncDrift(windowsPerStack, gate, maxDrift, driftDen, rounds int, refDelay, centre []int32) (*SyncLines, error) {
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(g.ctx, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	pairs, stations := int(C.tdoa_num_pairs(g.ctx)), len(refDelay)
	if int(total)*pairs == 0 || stations*(stations-1)/2 != pairs {
		return nil, fmt.Errorf("tdoa_process_sync_drift: no stacks, fewer than two stations, or not one delay per station")
	}
	o := newSyncLines(int(total), stations, pairs)
	if rc := C.tdoa_process_sync_drift(g.ctx, C.int(windowsPerStack), C.int(gate), C.int(maxDrift), C.int(driftDen), C.int(rounds),
		tablePtr(refDelay), centrePtr(centre), &o.Line[0], i32Ptr(o.Clock), i32Ptr(o.Rate), i32Ptr(o.Rows), i32Ptr(o.Lags),
		(*C.double)(unsafe.Pointer(&o.Corr[0]))); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_process_sync_drift: %s", C.GoString(C.tdoa_last_error(g.ctx)))
	}
	return o, nil
}

// SyncLineClock continues one line (clock in samples and rate, one per station) over positions first .. first + n - 1 in
// units of 1/16 sample: [position][station], what LocateSetClock takes.  Host only.
func SyncLineClock(clock, rate []int32, driftDen, first, n int) ([]int32, error) {
	if len(clock) == 0 || len(clock) != len(rate) || n < 1 {
		return nil, fmt.Errorf("tdoa_sync_line_clock: one clock and one rate per station, n >= 1")
	}
	out := make([]int32, n*len(clock))
	if rc := C.tdoa_sync_line_clock(i32Ptr(clock), i32Ptr(rate), C.int(len(clock)), C.int(driftDen), C.int(first), C.int(n), i32Ptr(out)); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_sync_line_clock: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	return out, nil
}

// SyncLinesFine is what ProcessSyncDriftFine returns: the coarse stage's outputs exactly as ProcessSyncDrift's, and the
// refinement's: one more record per block, Clock16 [3][station] in units of 1/16 sample, FineRate [3][station] in units of
// 1/(U driftDen) lag per stack, FineRows [stack][station] in units of 1/16 sample (what LocateSetClock takes for that block),
// FineLags [stack][pair] in units of 1/U sample and FineCorr, the signed value of the upsampled word there.
type SyncLinesFine struct {
	SyncLines
	Fine               []C.tdoa_sync_line
	Clock16, FineRate  []int32
	FineRows, FineLags []int32
	FineCorr           []float64
}

func newSyncLinesFine(total, stations, pairs int) *SyncLinesFine {
	return &SyncLinesFine{SyncLines: *newSyncLines(total, stations, pairs), Fine: make([]C.tdoa_sync_line, 3),
		Clock16: make([]int32, 3*stations), FineRate: make([]int32, 3*stations), FineRows: make([]int32, total*stations),
		FineLags: make([]int32, total*pairs), FineCorr: make([]float64, total*pairs)}
}

// ProcessSyncDriftFine is the fine clock lines (the header's "fine clock lines"): ProcessSyncDrift's search, then fineRounds
// sweeps that move every station's offset by up to u fine lags of 1/u sample and its rate by up to u steps of 1/(u driftDen)
// lag per stack (u one of 2, 4, 8, 16) on the words of the surfaces upsampled as LocateSetUpsample defines them, evaluated
// from Q without materialising them.  SyncLineClock16 continues a fine line past its block.
func (g *gpuCorrelator) ProcessSyncDriftFine(windowsPerStack, gate, maxDrift, driftDen, rounds, u, fineRounds int, refDelay, centre []int32) (*SyncLinesFine, error) {
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(g.ctx, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	pairs, stations := int(C.tdoa_num_pairs(g.ctx)), len(refDelay)
	if int(total)*pairs == 0 || stations*(stations-1)/2 != pairs {
		return nil, fmt.Errorf("tdoa_process_sync_drift_fine: no stacks, fewer than two stations, or not one delay per station")
	}
	o := newSyncLinesFine(int(total), stations, pairs)
	if rc := C.tdoa_process_sync_drift_fine(g.ctx, C.int(windowsPerStack), C.int(gate), C.int(maxDrift), C.int(driftDen), C.int(rounds),
		C.int(u), C.int(fineRounds), tablePtr(refDelay), centrePtr(centre), &o.Line[0], i32Ptr(o.Clock), i32Ptr(o.Rate), i32Ptr(o.Rows),
		i32Ptr(o.Lags), (*C.double)(unsafe.Pointer(&o.Corr[0])), &o.Fine[0], i32Ptr(o.Clock16), i32Ptr(o.FineRate), i32Ptr(o.FineRows),
		i32Ptr(o.FineLags), (*C.double)(unsafe.Pointer(&o.FineCorr[0]))); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_process_sync_drift_fine: %s", C.GoString(C.tdoa_last_error(g.ctx)))
	}
	return o, nil
}

// SyncLineClock16 continues one fine line (clock16 in units of 1/16 sample and the fine rate, one per station) over positions
// first .. first + n - 1 in units of 1/16 sample: [position][station], what LocateSetClock takes.  Host only.
func SyncLineClock16(clock16, fineRate []int32, u, driftDen, first, n int) ([]int32, error) {
	if len(clock16) == 0 || len(clock16) != len(fineRate) || n < 1 {
		return nil, fmt.Errorf("tdoa_sync_line_clock16: one clock and one rate per station, n >= 1")
	}
	out := make([]int32, n*len(clock16))
	if rc := C.tdoa_sync_line_clock16(i32Ptr(clock16), i32Ptr(fineRate), C.int(len(clock16)), C.int(u), C.int(driftDen), C.int(first), C.int(n),
		i32Ptr(out)); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_sync_line_clock16: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	return out, nil
}

// ClockMix is one entry of a clock mix (the header's tdoa_clock_mix): the row of a stack is the nearest integer to
// (Wa clock16[A] + Wb clock16[B]) / (Wa + Wb), halves away from zero.  {t, t, 1, 0} is stack t's own clock, {a, b, 1, 1} the
// midpoint of two stacks' clocks.
type ClockMix struct {
	A, B, Wa, Wb int32
}

func mixPtr(mix []ClockMix) *C.tdoa_clock_mix {
	if len(mix) == 0 {
		return nil
	}
	return (*C.tdoa_clock_mix)(unsafe.Pointer(&mix[0]))
}

// MidpointMix is the mix for [reference | target | reference] blocks of stacksPerBlock stacks: blocks 1 and 3 keep their own
// rows, stack j of block 2 gets the midpoint of stack j of blocks 1 and 3.
func MidpointMix(stacksPerBlock int) []ClockMix {
	l := int32(stacksPerBlock)
	mix := make([]ClockMix, 3*stacksPerBlock)
	for t := int32(0); t < 3*l; t++ {
		mix[t] = ClockMix{t, t, 1, 0}
		if t >= l && t < 2*l {
			mix[t] = ClockMix{t - l, t + l, 1, 1}
		}
	}
	return mix
}

// ClockMixRows is the mix in plain C (host only): clock16 [stack][station] in units of 1/16 sample and one entry per row ->
// [row][station], what LocateSetClock takes and what ProcessSyncLocate locates under.
func ClockMixRows(clock16 []int32, stations int, mix []ClockMix) ([]int32, error) {
	if stations < 1 || len(clock16) == 0 || len(clock16)%stations != 0 || len(mix) == 0 {
		return nil, fmt.Errorf("tdoa_clock_mix_rows: clock16 must be [stack][station] and the mix not empty")
	}
	out := make([]int32, len(mix)*stations)
	if rc := C.tdoa_clock_mix_rows(i32Ptr(clock16), C.int(len(clock16)/stations), C.int(stations), mixPtr(mix), C.int(len(mix)),
		i32Ptr(out)); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_clock_mix_rows: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	return out, nil
}

// SyncLocate is what ProcessSyncLocate returns: ProcessSyncFine's outputs, the stacks' clock rows [stack][station] in units of
// 1/16 sample, and ProcessLocateZoom's outputs under those rows.
type SyncLocate struct {
	SyncFine
	Rows []int32
	LocateZoom
}

// ProcessSyncLocate is the header's "clocks to fix in one call": the fine clock search, a clock row per stack mixed on the device
// from its clocks (mix: one entry per stack, nil: every stack its own clock; MidpointMix for the usual captures) and the zoom
// locate under those rows, in one step.  The clock table of LocateSetClock is neither read nor changed.
func (g *gpuCorrelator) ProcessSyncLocate(windowsPerStack, gate, rounds, u, fineRounds int, refDelay, centre []int32, mix []ClockMix,
	minSeparation, z, h, fineSeparation int) (*SyncLocate, error) {
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(g.ctx, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	pairs, stations := int(C.tdoa_num_pairs(g.ctx)), len(refDelay)
	if int(total)*pairs == 0 || stations*(stations-1)/2 != pairs || (mix != nil && len(mix) != int(total)) {
		return nil, fmt.Errorf("tdoa_process_sync_locate: no stacks, fewer than two stations, not one delay per station or not one mix entry per stack")
	}
	o := &SyncLocate{SyncFine: *newSyncFine(int(total), stations, pairs), Rows: make([]int32, int(total)*stations),
		LocateZoom: *newLocateZoom(int(total), pairs)}
	f, l := &o.SyncFine, &o.LocateZoom
	if rc := C.tdoa_process_sync_locate(g.ctx, C.int(windowsPerStack), C.int(gate), C.int(rounds), C.int(u), C.int(fineRounds), tablePtr(refDelay),
		centrePtr(centre), mixPtr(mix), C.int(minSeparation), C.int(z), C.int(h), C.int(fineSeparation), &f.Sync[0], i32Ptr(f.Clock),
		i32Ptr(f.Lags), (*C.double)(unsafe.Pointer(&f.Corr[0])), &f.Fine[0], i32Ptr(f.Clock16), i32Ptr(f.FineLags),
		(*C.double)(unsafe.Pointer(&f.FineCorr[0])), i32Ptr(o.Rows), &l.Loc[0], i32Ptr(l.Lags), (*C.double)(unsafe.Pointer(&l.Corr[0])), nil,
		&l.Zoom[0], i32Ptr(l.ZLags), (*C.double)(unsafe.Pointer(&l.ZCorr[0])), nil); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_process_sync_locate: %s", C.GoString(C.tdoa_last_error(g.ctx)))
	}
	return o, nil
}

// windowQuality is fastAnalyzeSamples' statistics (fast_analyzer.go:117-155) for every (window, station).
func (g *gpuCorrelator) windowQuality(stations int) ([]C.tdoa_window_quality, error) {
	var perBlock, total C.int
	C.tdoa_num_windows(g.ctx, &perBlock, &total)
	out := make([]C.tdoa_window_quality, int(total)*stations)
	if rc := C.tdoa_window_quality_all(g.ctx, 0, 1, &out[0]); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_window_quality_all: %s", C.GoString(C.tdoa_last_error(g.ctx)))
	}
	return out, nil
}

// Group shards the batched path over several GPUs in one call: one tdoa_ctx per member, member k = rank k of
// len(devices). Devices may repeat (several members on one GPU). Not safe for concurrent use; the library runs the
// members on threads of its own inside each call and merges their peaks on the host.
type Group struct{ g *C.tdoa_group }

// NewGroup opens one context per entry of devices (e.g. 0..tdoa_device_count()-1 for the whole node).
func NewGroup(devices []int32, goLagSet bool) (*Group, error) {
	if len(devices) == 0 {
		return nil, fmt.Errorf("tdoa_group_create: no devices")
	}
	var p C.tdoa_params
	C.tdoa_default_params(&p)
	if goLagSet {
		p.lag_mode = C.TDOA_LAGS_GO
	}
	var g *C.tdoa_group
	rc := C.tdoa_group_create(&p, (*C.int32_t)(unsafe.Pointer(&devices[0])), C.int(len(devices)), &g)
	if rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_group_create: %s (%s)", C.GoString(C.tdoa_strerror(rc)),
			C.GoString(C.tdoa_group_last_error(nil)))
	}
	return &Group{g: g}, nil
}

func (g *Group) Close() { C.tdoa_group_destroy(g.g) }

// UploadFiles hands the group one .dat file per station (paths[s] = station s); every member reads only the sample
// runs of the windows it owns. Returns size/2 per file, like loadIQData (processor.go:182).
func (g *Group) UploadFiles(paths []string) ([]int, error) {
	if len(paths) == 0 {
		return nil, fmt.Errorf("tdoa_group_capture_upload_files: no files")
	}
	cpaths := make([]*C.char, len(paths)) // C strings: the slice holds no Go pointers (cgo rule)
	for i, p := range paths {
		cpaths[i] = C.CString(p)
		defer C.free(unsafe.Pointer(cpaths[i]))
	}
	ns := make([]C.size_t, len(paths))
	if rc := C.tdoa_group_capture_upload_files(g.g, C.int(len(paths)), &cpaths[0], &ns[0]); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_group_capture_upload_files: %s", C.GoString(C.tdoa_group_last_error(g.g)))
	}
	out := make([]int, len(ns))
	for i, n := range ns {
		out[i] = int(n)
	}
	return out, nil
}

// Process is processCaptures over the group: one peak per (window, pair), pairs ordered i<j, the same bytes one context
// returns.
func (g *Group) Process() ([]C.tdoa_peak, int, error) {
	m := C.tdoa_group_member(g.g, 0)
	var perBlock, total C.int
	if rc := C.tdoa_num_windows(m, &perBlock, &total); rc != C.TDOA_OK {
		return nil, 0, fmt.Errorf("tdoa_num_windows: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	pairs := int(C.tdoa_num_pairs(m))
	out := make([]C.tdoa_peak, int(total)*pairs)
	if rc := C.tdoa_group_process(g.g, &out[0]); rc != C.TDOA_OK {
		return nil, 0, fmt.Errorf("tdoa_group_process: %s", C.GoString(C.tdoa_group_last_error(g.g)))
	}
	return out, pairs, nil
}

// ProcessStacked is gpuCorrelator.ProcessStacked over the group: the members' fixed-point partial sums are added on the
// host and finished on member 0, the same bytes one context returns.
func (g *Group) ProcessStacked(windowsPerStack, k, minSeparation int, gate float64) ([]C.tdoa_peak, []C.int32_t, []C.tdoa_fine_peak, error) {
	m := C.tdoa_group_member(g.g, 0)
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(m, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, nil, nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	n := int(total) * int(C.tdoa_num_pairs(m))
	if n == 0 || k < 1 {
		return nil, nil, nil, fmt.Errorf("tdoa_group_process_stacked: no stack-pairs or k < 1")
	}
	peaks, count, fine := make([]C.tdoa_peak, n*k), make([]C.int32_t, n), make([]C.tdoa_fine_peak, n)
	if rc := C.tdoa_group_process_stacked(g.g, C.int(windowsPerStack), C.int(k), C.int(minSeparation), C.double(gate),
		&peaks[0], &count[0], &fine[0], nil); rc != C.TDOA_OK {
		return nil, nil, nil, fmt.Errorf("tdoa_group_process_stacked: %s", C.GoString(C.tdoa_group_last_error(g.g)))
	}
	return peaks, count, fine, nil
}

// ProcessClosure is gpuCorrelator.ProcessClosure over the group: the members' fixed-point partial sums are added on the
// host and searched on member 0, the same bytes one context returns.
func (g *Group) ProcessClosure(windowsPerStack, gate, minSeparation int, centre []int32) ([]C.tdoa_closure, int, error) {
	m := C.tdoa_group_member(g.g, 0)
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(m, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, 0, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	triples := int(C.tdoa_num_triples(m))
	if int(total)*triples == 0 {
		return nil, 0, fmt.Errorf("tdoa_group_process_closure: no stacks or fewer than three stations")
	}
	out := make([]C.tdoa_closure, int(total)*triples)
	if rc := C.tdoa_group_process_closure(g.g, C.int(windowsPerStack), C.int(gate), C.int(minSeparation), centrePtr(centre), &out[0]); rc != C.TDOA_OK {
		return nil, 0, fmt.Errorf("tdoa_group_process_closure: %s", C.GoString(C.tdoa_group_last_error(g.g)))
	}
	return out, triples, nil
}

// LocateSetTable hands every member the delay table (gpuCorrelator.LocateSetTable).
func (g *Group) LocateSetTable(delay []int32, nCells, nCols, nStations int) error {
	if rc := C.tdoa_group_locate_set_table(g.g, tablePtr(delay), C.int(nCells), C.int(nCols), C.int(nStations)); rc != C.TDOA_OK {
		return fmt.Errorf("tdoa_group_locate_set_table: %s", C.GoString(C.tdoa_group_last_error(g.g)))
	}
	return nil
}

// LocateSetFineTable hands every member the zoom locate's fine table (gpuCorrelator.LocateSetFineTable).
func (g *Group) LocateSetFineTable(delay []int32, nCells, nCols, nStations int) error {
	if rc := C.tdoa_group_locate_set_fine_table(g.g, tablePtr(delay), C.int(nCells), C.int(nCols), C.int(nStations)); rc != C.TDOA_OK {
		return fmt.Errorf("tdoa_group_locate_set_fine_table: %s", C.GoString(C.tdoa_group_last_error(g.g)))
	}
	return nil
}

// ProcessLocateZoom is gpuCorrelator.ProcessLocateZoom over the group: the members' fixed-point partial sums are added on the
// host and searched on member 0, coarse stage and window, the same bytes one context returns.
func (g *Group) ProcessLocateZoom(windowsPerStack, minSeparation, z, h, fineSeparation int) (*LocateZoom, error) {
	m := C.tdoa_group_member(g.g, 0)
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(m, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	pairs := int(C.tdoa_num_pairs(m))
	if int(total)*pairs == 0 {
		return nil, fmt.Errorf("tdoa_group_process_locate_zoom: no stacks or fewer than two stations")
	}
	o := newLocateZoom(int(total), pairs)
	if rc := C.tdoa_group_process_locate_zoom(g.g, C.int(windowsPerStack), C.int(minSeparation), C.int(z), C.int(h), C.int(fineSeparation),
		&o.Loc[0], (*C.int32_t)(unsafe.Pointer(&o.Lags[0])), (*C.double)(unsafe.Pointer(&o.Corr[0])), nil,
		&o.Zoom[0], (*C.int32_t)(unsafe.Pointer(&o.ZLags[0])), (*C.double)(unsafe.Pointer(&o.ZCorr[0])), nil); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_group_process_locate_zoom: %s", C.GoString(C.tdoa_group_last_error(g.g)))
	}
	return o, nil
}

// ProcessLocateMultiZoom is gpuCorrelator.ProcessLocateMultiZoom over the group: the members' fixed-point partial sums are
// added on the host and searched on member 0, rounds and windows, the same bytes one context returns.
func (g *Group) ProcessLocateMultiZoom(windowsPerStack, nEmitters, guard, minSeparation, z, h, fineSeparation int) (*LocateMultiZoom, error) {
	m := C.tdoa_group_member(g.g, 0)
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(m, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	pairs := int(C.tdoa_num_pairs(m))
	if int(total)*pairs == 0 || nEmitters < 1 || nEmitters > 8 {
		return nil, fmt.Errorf("tdoa_group_process_locate_multi_zoom: no stacks, fewer than two stations or nEmitters outside 1 .. 8")
	}
	o := newLocateMultiZoom(nEmitters, int(total), pairs)
	if rc := C.tdoa_group_process_locate_multi_zoom(g.g, C.int(windowsPerStack), C.int(nEmitters), C.int(guard), C.int(minSeparation), C.int(z),
		C.int(h), C.int(fineSeparation), &o.Loc[0], (*C.int32_t)(unsafe.Pointer(&o.Lags[0])), (*C.double)(unsafe.Pointer(&o.Corr[0])), nil,
		&o.Zoom[0], (*C.int32_t)(unsafe.Pointer(&o.ZPairs[0])), (*C.int32_t)(unsafe.Pointer(&o.ZLags[0])),
		(*C.double)(unsafe.Pointer(&o.ZCorr[0])), nil); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_group_process_locate_multi_zoom: %s", C.GoString(C.tdoa_group_last_error(g.g)))
	}
	return o, nil
}

// ProcessLocate is gpuCorrelator.ProcessLocate over the group: the members' fixed-point partial sums are added on the host
// and searched on member 0, the same bytes one context returns.
func (g *Group) ProcessLocate(windowsPerStack, minSeparation int) (loc []C.tdoa_location, lags []int32, corr []float64, err error) {
	m := C.tdoa_group_member(g.g, 0)
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(m, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, nil, nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	pairs := int(C.tdoa_num_pairs(m))
	if int(total)*pairs == 0 {
		return nil, nil, nil, fmt.Errorf("tdoa_group_process_locate: no stacks or fewer than two stations")
	}
	loc = make([]C.tdoa_location, int(total))
	lags = make([]int32, int(total)*pairs)
	corr = make([]float64, int(total)*pairs)
	if rc := C.tdoa_group_process_locate(g.g, C.int(windowsPerStack), C.int(minSeparation), &loc[0], (*C.int32_t)(unsafe.Pointer(&lags[0])),
		(*C.double)(unsafe.Pointer(&corr[0])), nil); rc != C.TDOA_OK {
		return nil, nil, nil, fmt.Errorf("tdoa_group_process_locate: %s", C.GoString(C.tdoa_group_last_error(g.g)))
	}
	return loc, lags, corr, nil
}

// ProcessLocateMulti is gpuCorrelator.ProcessLocateMulti over the group: the members' fixed-point partial sums are added on
// the host and searched on member 0, the same bytes one context returns.
func (g *Group) ProcessLocateMulti(windowsPerStack, nEmitters, guard, minSeparation int) (loc []C.tdoa_location, lags []int32, corr []float64, err error) {
	m := C.tdoa_group_member(g.g, 0)
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(m, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, nil, nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	pairs := int(C.tdoa_num_pairs(m))
	if int(total)*pairs == 0 || nEmitters < 1 {
		return nil, nil, nil, fmt.Errorf("tdoa_group_process_locate_multi: no stacks, fewer than two stations or no rounds")
	}
	loc = make([]C.tdoa_location, nEmitters*int(total))
	lags = make([]int32, nEmitters*int(total)*pairs)
	corr = make([]float64, nEmitters*int(total)*pairs)
	if rc := C.tdoa_group_process_locate_multi(g.g, C.int(windowsPerStack), C.int(nEmitters), C.int(guard), C.int(minSeparation), &loc[0],
		(*C.int32_t)(unsafe.Pointer(&lags[0])), (*C.double)(unsafe.Pointer(&corr[0])), nil); rc != C.TDOA_OK {
		return nil, nil, nil, fmt.Errorf("tdoa_group_process_locate_multi: %s", C.GoString(C.tdoa_group_last_error(g.g)))
	}
	return loc, lags, corr, nil
}

// ProcessLocateTrack is gpuCorrelator.ProcessLocateTrack over the group: the members' fixed-point partial sums are added on
// the host and searched on member 0, the same bytes one context returns.
func (g *Group) ProcessLocateTrack(windowsPerStack, maxStep, minSeparation int) (track []C.tdoa_cell_track, cells []int32, own []int64, lags []int32, corr []float64, err error) {
	m := C.tdoa_group_member(g.g, 0)
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(m, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, nil, nil, nil, nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	pairs := int(C.tdoa_num_pairs(m))
	if int(total)*pairs == 0 {
		return nil, nil, nil, nil, nil, fmt.Errorf("tdoa_group_process_locate_track: no stacks or fewer than two stations")
	}
	track = make([]C.tdoa_cell_track, int(total)/int(perBlock))
	cells = make([]int32, int(total))
	own = make([]int64, int(total))
	lags = make([]int32, int(total)*pairs)
	corr = make([]float64, int(total)*pairs)
	if rc := C.tdoa_group_process_locate_track(g.g, C.int(windowsPerStack), C.int(maxStep), C.int(minSeparation), &track[0],
		(*C.int32_t)(unsafe.Pointer(&cells[0])), (*C.int64_t)(unsafe.Pointer(&own[0])), (*C.int32_t)(unsafe.Pointer(&lags[0])),
		(*C.double)(unsafe.Pointer(&corr[0])), nil); rc != C.TDOA_OK {
		return nil, nil, nil, nil, nil, fmt.Errorf("tdoa_group_process_locate_track: %s", C.GoString(C.tdoa_group_last_error(g.g)))
	}
	return track, cells, own, lags, corr, nil
}

// ProcessLocateTrackMulti is gpuCorrelator.ProcessLocateTrackMulti over the group: the members' fixed-point partial sums are
// added on the host and tracked on member 0, the same bytes one context returns.
func (g *Group) ProcessLocateTrackMulti(windowsPerStack, maxStep, nEmitters, guard, minSeparation int) (*TrackRounds, error) {
	m := C.tdoa_group_member(g.g, 0)
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(m, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	pairs := int(C.tdoa_num_pairs(m))
	if int(total)*pairs == 0 || nEmitters < 1 {
		return nil, fmt.Errorf("tdoa_group_process_locate_track_multi: no stacks, fewer than two stations or no rounds")
	}
	r := newTrackRounds(nEmitters, int(total), int(perBlock), pairs)
	if rc := C.tdoa_group_process_locate_track_multi(g.g, C.int(windowsPerStack), C.int(maxStep), C.int(nEmitters), C.int(guard),
		C.int(minSeparation), &r.Track[0], (*C.int32_t)(unsafe.Pointer(&r.Cells[0])), (*C.int64_t)(unsafe.Pointer(&r.Own[0])),
		(*C.int32_t)(unsafe.Pointer(&r.Pairs[0])), (*C.int32_t)(unsafe.Pointer(&r.Lags[0])), (*C.double)(unsafe.Pointer(&r.Corr[0])),
		nil); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_group_process_locate_track_multi: %s", C.GoString(C.tdoa_group_last_error(g.g)))
	}
	return r, nil
}

// LocateSetClock hands every member the stations' clocks (gpuCorrelator.LocateSetClock).
func (g *Group) LocateSetClock(clock []int32, nStacks, nStations int) error {
	if rc := C.tdoa_group_locate_set_clock(g.g, tablePtr(clock), C.int(nStacks), C.int(nStations)); rc != C.TDOA_OK {
		return fmt.Errorf("tdoa_group_locate_set_clock: %s", C.GoString(C.tdoa_group_last_error(g.g)))
	}
	return nil
}

// LocateSetStats switches every member's map statistics on or off (gpuCorrelator.LocateSetStats).
func (g *Group) LocateSetStats(ranks []uint16, foot int) error {
	var p *C.uint16_t
	if len(ranks) > 0 {
		p = (*C.uint16_t)(unsafe.Pointer(&ranks[0]))
	}
	if rc := C.tdoa_group_locate_set_stats(g.g, p, C.int(len(ranks)), C.int(foot)); rc != C.TDOA_OK {
		return fmt.Errorf("tdoa_group_locate_set_stats: %s", C.GoString(C.tdoa_group_last_error(g.g)))
	}
	return nil
}

// LocateLastStats is gpuCorrelator.LocateLastStats for the group's last call: the same bytes one context returns.
func (g *Group) LocateLastStats() ([]C.tdoa_map_stats, error) {
	var n C.int
	C.tdoa_group_locate_last_stats(g.g, nil, 0, &n)
	out := make([]C.tdoa_map_stats, int(n)+1)
	if rc := C.tdoa_group_locate_last_stats(g.g, &out[0], n, &n); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_group_locate_last_stats: %s", C.GoString(C.tdoa_group_last_error(g.g)))
	}
	return out[:int(n)], nil
}

// LocateSetUpsample sets every member's lag grid (gpuCorrelator.LocateSetUpsample); a group of several upsamples the merged
// sum on member 0.
func (g *Group) LocateSetUpsample(u int) error {
	if rc := C.tdoa_group_locate_set_upsample(g.g, C.int(u)); rc != C.TDOA_OK {
		return fmt.Errorf("tdoa_group_locate_set_upsample: %s", C.GoString(C.tdoa_group_last_error(g.g)))
	}
	return nil
}

// ProcessSync is gpuCorrelator.ProcessSync over the group: the members' fixed-point partial sums are added on the host and
// searched on member 0, the same bytes one context returns.
func (g *Group) ProcessSync(windowsPerStack, gate, rounds int, refDelay, centre []int32) (sync []C.tdoa_sync, clock, lags []int32, corr []float64, err error) {
	m := C.tdoa_group_member(g.g, 0)
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(m, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, nil, nil, nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	pairs, stations := int(C.tdoa_num_pairs(m)), len(refDelay)
	if int(total)*pairs == 0 || stations*(stations-1)/2 != pairs {
		return nil, nil, nil, nil, fmt.Errorf("tdoa_group_process_sync: no stacks, fewer than two stations, or not one delay per station")
	}
	sync = make([]C.tdoa_sync, int(total))
	clock = make([]int32, int(total)*stations)
	lags = make([]int32, int(total)*pairs)
	corr = make([]float64, int(total)*pairs)
	if rc := C.tdoa_group_process_sync(g.g, C.int(windowsPerStack), C.int(gate), C.int(rounds), tablePtr(refDelay), centrePtr(centre), &sync[0],
		(*C.int32_t)(unsafe.Pointer(&clock[0])), (*C.int32_t)(unsafe.Pointer(&lags[0])), (*C.double)(unsafe.Pointer(&corr[0]))); rc != C.TDOA_OK {
		return nil, nil, nil, nil, fmt.Errorf("tdoa_group_process_sync: %s", C.GoString(C.tdoa_group_last_error(g.g)))
	}
	return sync, clock, lags, corr, nil
}

// ProcessSyncFine is gpuCorrelator.ProcessSyncFine over the group: the members' fixed-point partial sums are added on the host
// and searched on member 0, coarse stage and refinement, the same bytes one context returns.
func (g *Group) ProcessSyncFine(windowsPerStack, gate, rounds, u, fineRounds int, refDelay, centre []int32) (*SyncFine, error) {
	m := C.tdoa_group_member(g.g, 0)
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(m, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	pairs, stations := int(C.tdoa_num_pairs(m)), len(refDelay)
	if int(total)*pairs == 0 || stations*(stations-1)/2 != pairs {
		return nil, fmt.Errorf("tdoa_group_process_sync_fine: no stacks, fewer than two stations, or not one delay per station")
	}
	o := newSyncFine(int(total), stations, pairs)
	if rc := C.tdoa_group_process_sync_fine(g.g, C.int(windowsPerStack), C.int(gate), C.int(rounds), C.int(u), C.int(fineRounds), tablePtr(refDelay),
		centrePtr(centre), &o.Sync[0], (*C.int32_t)(unsafe.Pointer(&o.Clock[0])), (*C.int32_t)(unsafe.Pointer(&o.Lags[0])),
		(*C.double)(unsafe.Pointer(&o.Corr[0])), &o.Fine[0], (*C.int32_t)(unsafe.Pointer(&o.Clock16[0])),
		(*C.int32_t)(unsafe.Pointer(&o.FineLags[0])), (*C.double)(unsafe.Pointer(&o.FineCorr[0]))); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_group_process_sync_fine: %s", C.GoString(C.tdoa_group_last_error(g.g)))
	}
	return o, nil
}

// ProcessSyncLocate is gpuCorrelator.ProcessSyncLocate over the group: the members' fixed-point partial sums are added on the
// host and searched on member 0 with its table, fine table and settings, the same bytes one context returns.
func (g *Group) ProcessSyncLocate(windowsPerStack, gate, rounds, u, fineRounds int, refDelay, centre []int32, mix []ClockMix,
	minSeparation, z, h, fineSeparation int) (*SyncLocate, error) {
	m := C.tdoa_group_member(g.g, 0)
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(m, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	pairs, stations := int(C.tdoa_num_pairs(m)), len(refDelay)
	if int(total)*pairs == 0 || stations*(stations-1)/2 != pairs || (mix != nil && len(mix) != int(total)) {
		return nil, fmt.Errorf("tdoa_group_process_sync_locate: no stacks, fewer than two stations, not one delay per station or not one mix entry per stack")
	}
	o := &SyncLocate{SyncFine: *newSyncFine(int(total), stations, pairs), Rows: make([]int32, int(total)*stations),
		LocateZoom: *newLocateZoom(int(total), pairs)}
	f, l := &o.SyncFine, &o.LocateZoom
	if rc := C.tdoa_group_process_sync_locate(g.g, C.int(windowsPerStack), C.int(gate), C.int(rounds), C.int(u), C.int(fineRounds),
		tablePtr(refDelay), centrePtr(centre), mixPtr(mix), C.int(minSeparation), C.int(z), C.int(h), C.int(fineSeparation), &f.Sync[0],
		i32Ptr(f.Clock), i32Ptr(f.Lags), (*C.double)(unsafe.Pointer(&f.Corr[0])), &f.Fine[0], i32Ptr(f.Clock16), i32Ptr(f.FineLags),
		(*C.double)(unsafe.Pointer(&f.FineCorr[0])), i32Ptr(o.Rows), &l.Loc[0], i32Ptr(l.Lags), (*C.double)(unsafe.Pointer(&l.Corr[0])), nil,
		&l.Zoom[0], i32Ptr(l.ZLags), (*C.double)(unsafe.Pointer(&l.ZCorr[0])), nil); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_group_process_sync_locate: %s", C.GoString(C.tdoa_group_last_error(g.g)))
	}
	return o, nil
}

// ProcessSyncDrift is gpuCorrelator.ProcessSyncDrift over the group: the members' fixed-point partial sums are added on the
// host and searched on member 0, the same bytes one context returns.
func (g *Group) ProcessSyncDrift(windowsPerStack, gate, maxDrift, driftDen, rounds int, refDelay, centre []int32) (*SyncLines, error) {
	m := C.tdoa_group_member(g.g, 0)
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(m, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	pairs, stations := int(C.tdoa_num_pairs(m)), len(refDelay)
	if int(total)*pairs == 0 || stations*(stations-1)/2 != pairs {
		return nil, fmt.Errorf("tdoa_group_process_sync_drift: no stacks, fewer than two stations, or not one delay per station")
	}
	o := newSyncLines(int(total), stations, pairs)
	if rc := C.tdoa_group_process_sync_drift(g.g, C.int(windowsPerStack), C.int(gate), C.int(maxDrift), C.int(driftDen), C.int(rounds),
		tablePtr(refDelay), centrePtr(centre), &o.Line[0], i32Ptr(o.Clock), i32Ptr(o.Rate), i32Ptr(o.Rows), i32Ptr(o.Lags),
		(*C.double)(unsafe.Pointer(&o.Corr[0]))); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_group_process_sync_drift: %s", C.GoString(C.tdoa_group_last_error(g.g)))
	}
	return o, nil
}

// ProcessSyncDriftFine is gpuCorrelator.ProcessSyncDriftFine over the group: the members' fixed-point partial sums are added on
// the host and searched on member 0, coarse stage and refinement, the same bytes one context returns.
func (g *Group) ProcessSyncDriftFine(windowsPerStack, gate, maxDrift, driftDen, rounds, u, fineRounds int, refDelay, centre []int32) (*SyncLinesFine, error) {
	m := C.tdoa_group_member(g.g, 0)
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(m, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	pairs, stations := int(C.tdoa_num_pairs(m)), len(refDelay)
	if int(total)*pairs == 0 || stations*(stations-1)/2 != pairs {
		return nil, fmt.Errorf("tdoa_group_process_sync_drift_fine: no stacks, fewer than two stations, or not one delay per station")
	}
	o := newSyncLinesFine(int(total), stations, pairs)
	if rc := C.tdoa_group_process_sync_drift_fine(g.g, C.int(windowsPerStack), C.int(gate), C.int(maxDrift), C.int(driftDen), C.int(rounds),
		C.int(u), C.int(fineRounds), tablePtr(refDelay), centrePtr(centre), &o.Line[0], i32Ptr(o.Clock), i32Ptr(o.Rate), i32Ptr(o.Rows),
		i32Ptr(o.Lags), (*C.double)(unsafe.Pointer(&o.Corr[0])), &o.Fine[0], i32Ptr(o.Clock16), i32Ptr(o.FineRate), i32Ptr(o.FineRows),
		i32Ptr(o.FineLags), (*C.double)(unsafe.Pointer(&o.FineCorr[0]))); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_group_process_sync_drift_fine: %s", C.GoString(C.tdoa_group_last_error(g.g)))
	}
	return o, nil
}

// LocateTrackZoom is what ProcessLocateTrackZoom returns: the coarse stage's outputs exactly as ProcessLocateTrack's (Track, Cells,
// Own, Lags, Corr), and per block the track through the fine table's windows: its record (ZTrack: the cells are fine cells), its
// fine cell in every stack and that stack's own score there (ZCells, ZOwn: [block][stacks per block]), and the fine cells' lags
// (1/u sample with LocateSetUpsample) and signed correlations (ZLags, ZCorr: [stack][pair]).
type LocateTrackZoom struct {
	Track  []C.tdoa_cell_track
	Cells  []int32
	Own    []int64
	Lags   []int32
	Corr   []float64
	ZTrack []C.tdoa_cell_track
	ZCells []int32
	ZOwn   []int64
	ZLags  []int32
	ZCorr  []float64
}

func newLocateTrackZoom(stacks, perBlock, pairs int) *LocateTrackZoom {
	return &LocateTrackZoom{Track: make([]C.tdoa_cell_track, stacks/perBlock), Cells: make([]int32, stacks), Own: make([]int64, stacks),
		Lags: make([]int32, stacks*pairs), Corr: make([]float64, stacks*pairs), ZTrack: make([]C.tdoa_cell_track, stacks/perBlock),
		ZCells: make([]int32, stacks), ZOwn: make([]int64, stacks), ZLags: make([]int32, stacks*pairs), ZCorr: make([]float64, stacks*pairs)}
}

// ProcessLocateTrackZoom is the zoomed cell track (the header's "zoomed cell tracks"): ProcessLocateTrack's tracks, then per block
// the track through the (2h+1)^2-cell windows of the fine table around z x the coarse track's cells, consecutive fine cells at
// most fineStep rows and columns apart, in the same step.  A fine cell's position is the caller's: row = cell / nCols of the fine
// table, col = the remainder.
func (g *gpuCorrelator) ProcessLocateTrackZoom(windowsPerStack, maxStep, minSeparation, z, h, fineStep, fineSeparation int) (*LocateTrackZoom, error) {
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(g.ctx, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	pairs := int(C.tdoa_num_pairs(g.ctx))
	if int(total)*pairs == 0 {
		return nil, fmt.Errorf("tdoa_process_locate_track_zoom: no stacks or fewer than two stations")
	}
	o := newLocateTrackZoom(int(total), int(perBlock), pairs)
	if rc := C.tdoa_process_locate_track_zoom(g.ctx, C.int(windowsPerStack), C.int(maxStep), C.int(minSeparation), C.int(z), C.int(h),
		C.int(fineStep), C.int(fineSeparation), &o.Track[0], (*C.int32_t)(unsafe.Pointer(&o.Cells[0])), (*C.int64_t)(unsafe.Pointer(&o.Own[0])),
		(*C.int32_t)(unsafe.Pointer(&o.Lags[0])), (*C.double)(unsafe.Pointer(&o.Corr[0])), nil,
		&o.ZTrack[0], (*C.int32_t)(unsafe.Pointer(&o.ZCells[0])), (*C.int64_t)(unsafe.Pointer(&o.ZOwn[0])),
		(*C.int32_t)(unsafe.Pointer(&o.ZLags[0])), (*C.double)(unsafe.Pointer(&o.ZCorr[0])), nil, nil); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_process_locate_track_zoom: %s", C.GoString(C.tdoa_last_error(g.ctx)))
	}
	return o, nil
}

// ProcessLocateTrackZoom is gpuCorrelator.ProcessLocateTrackZoom over the group: the members' fixed-point partial sums are added
// on the host and tracked on member 0, coarse tracks and windows, the same bytes one context returns.
func (g *Group) ProcessLocateTrackZoom(windowsPerStack, maxStep, minSeparation, z, h, fineStep, fineSeparation int) (*LocateTrackZoom, error) {
	m := C.tdoa_group_member(g.g, 0)
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(m, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	pairs := int(C.tdoa_num_pairs(m))
	if int(total)*pairs == 0 {
		return nil, fmt.Errorf("tdoa_group_process_locate_track_zoom: no stacks or fewer than two stations")
	}
	o := newLocateTrackZoom(int(total), int(perBlock), pairs)
	if rc := C.tdoa_group_process_locate_track_zoom(g.g, C.int(windowsPerStack), C.int(maxStep), C.int(minSeparation), C.int(z), C.int(h),
		C.int(fineStep), C.int(fineSeparation), &o.Track[0], (*C.int32_t)(unsafe.Pointer(&o.Cells[0])), (*C.int64_t)(unsafe.Pointer(&o.Own[0])),
		(*C.int32_t)(unsafe.Pointer(&o.Lags[0])), (*C.double)(unsafe.Pointer(&o.Corr[0])), nil,
		&o.ZTrack[0], (*C.int32_t)(unsafe.Pointer(&o.ZCells[0])), (*C.int64_t)(unsafe.Pointer(&o.ZOwn[0])),
		(*C.int32_t)(unsafe.Pointer(&o.ZLags[0])), (*C.double)(unsafe.Pointer(&o.ZCorr[0])), nil, nil); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_group_process_locate_track_zoom: %s", C.GoString(C.tdoa_group_last_error(g.g)))
	}
	return o, nil
}

// LineMix is one entry of a line mix (the header's tdoa_line_mix): the row of a stack is the nearest integer to
// (Wa cont(A, Xa) + Wb cont(B, Xb)) / (Wa + Wb), halves away from zero, cont(l, x) being fine line l continued to position x by
// SyncLineClock16's rule, x of either sign.  {l, x, l, x, 1, 0} is line l continued to x.
type LineMix struct {
	A, Xa, B, Xb, Wa, Wb int32
}

func lineMixPtr(mix []LineMix) *C.tdoa_line_mix {
	if len(mix) == 0 {
		return nil
	}
	return (*C.tdoa_line_mix)(unsafe.Pointer(&mix[0]))
}

// ForwardMix is the mix for [reference | target | reference] blocks of stacksPerBlock stacks: blocks 1 and 3 keep their own
// lines at their own positions, stack j of block 2 gets block 1's line continued to stacksPerBlock + j.
func ForwardMix(stacksPerBlock int) []LineMix {
	l := int32(stacksPerBlock)
	mix := make([]LineMix, 3*stacksPerBlock)
	for t := int32(0); t < 3*l; t++ {
		mix[t] = LineMix{t / l, t % l, t / l, t % l, 1, 0}
		if t >= l && t < 2*l {
			mix[t] = LineMix{0, t, 0, t, 1, 0}
		}
	}
	return mix
}

// LineMixRows is the line mix in plain C (host only): clock16 and fineRate [line][station] (1/16 sample; 1/(u driftDen) lag per
// position) and one entry per row -> [row][station], what LocateSetClock takes and what ProcessSyncDriftLocate tracks under.
func LineMixRows(clock16, fineRate []int32, stations, u, driftDen int, mix []LineMix) ([]int32, error) {
	if stations < 1 || len(clock16) == 0 || len(clock16)%stations != 0 || len(fineRate) != len(clock16) || len(mix) == 0 {
		return nil, fmt.Errorf("tdoa_line_mix_rows: clock16 and fineRate must be [line][station] and the mix not empty")
	}
	out := make([]int32, len(mix)*stations)
	if rc := C.tdoa_line_mix_rows(i32Ptr(clock16), i32Ptr(fineRate), C.int(len(clock16)/stations), C.int(stations), C.int(u), C.int(driftDen),
		lineMixPtr(mix), C.int(len(mix)), i32Ptr(out)); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_line_mix_rows: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	return out, nil
}

// SyncDriftLocate is what ProcessSyncDriftLocate returns: ProcessSyncDriftFine's outputs, the stacks' clock rows [stack][station]
// in units of 1/16 sample, and ProcessLocateTrackZoom's outputs under those rows.
type SyncDriftLocate struct {
	SyncLinesFine
	MixRows []int32
	LocateTrackZoom
}

func newSyncDriftLocate(total, perBlock, stations, pairs int) *SyncDriftLocate {
	return &SyncDriftLocate{SyncLinesFine: *newSyncLinesFine(total, stations, pairs), MixRows: make([]int32, total*stations),
		LocateTrackZoom: *newLocateTrackZoom(total, perBlock, pairs)}
}

// ProcessSyncDriftLocate is the header's "free-running clocks to fix in one call": the fine clock lines, a clock row per stack made
// on the device from their clocks and rates (mix: one entry per stack, nil: every stack its own line at its own position;
// ForwardMix for the usual captures) and the zoomed cell tracks under those rows, in one step.  The clock table of LocateSetClock
// is neither read nor changed.
func (g *gpuCorrelator) ProcessSyncDriftLocate(windowsPerStack, gate, maxDrift, driftDen, rounds, u, fineRounds int, refDelay, centre []int32,
	mix []LineMix, maxStep, minSeparation, z, h, fineStep, fineSeparation int) (*SyncDriftLocate, error) {
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(g.ctx, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	pairs, stations := int(C.tdoa_num_pairs(g.ctx)), len(refDelay)
	if int(total)*pairs == 0 || stations*(stations-1)/2 != pairs || (mix != nil && len(mix) != int(total)) {
		return nil, fmt.Errorf("tdoa_process_sync_drift_locate: no stacks, fewer than two stations, not one delay per station or not one mix entry per stack")
	}
	o := newSyncDriftLocate(int(total), int(perBlock), stations, pairs)
	f, l := &o.SyncLinesFine, &o.LocateTrackZoom
	if rc := C.tdoa_process_sync_drift_locate(g.ctx, C.int(windowsPerStack), C.int(gate), C.int(maxDrift), C.int(driftDen), C.int(rounds),
		C.int(u), C.int(fineRounds), tablePtr(refDelay), centrePtr(centre), lineMixPtr(mix), C.int(maxStep), C.int(minSeparation), C.int(z),
		C.int(h), C.int(fineStep), C.int(fineSeparation), &f.Line[0], i32Ptr(f.Clock), i32Ptr(f.Rate), i32Ptr(f.Rows), i32Ptr(f.Lags),
		(*C.double)(unsafe.Pointer(&f.Corr[0])), &f.Fine[0], i32Ptr(f.Clock16), i32Ptr(f.FineRate), i32Ptr(f.FineRows), i32Ptr(f.FineLags),
		(*C.double)(unsafe.Pointer(&f.FineCorr[0])), i32Ptr(o.MixRows), &l.Track[0], i32Ptr(l.Cells), (*C.int64_t)(unsafe.Pointer(&l.Own[0])),
		i32Ptr(l.Lags), (*C.double)(unsafe.Pointer(&l.Corr[0])), nil, &l.ZTrack[0], i32Ptr(l.ZCells), (*C.int64_t)(unsafe.Pointer(&l.ZOwn[0])),
		i32Ptr(l.ZLags), (*C.double)(unsafe.Pointer(&l.ZCorr[0])), nil, nil); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_process_sync_drift_locate: %s", C.GoString(C.tdoa_last_error(g.ctx)))
	}
	return o, nil
}

// ProcessSyncDriftLocate is gpuCorrelator.ProcessSyncDriftLocate over the group: the members' fixed-point partial sums are added
// on the host and searched on member 0 with its table, fine table and settings, the same bytes one context returns.
func (g *Group) ProcessSyncDriftLocate(windowsPerStack, gate, maxDrift, driftDen, rounds, u, fineRounds int, refDelay, centre []int32,
	mix []LineMix, maxStep, minSeparation, z, h, fineStep, fineSeparation int) (*SyncDriftLocate, error) {
	m := C.tdoa_group_member(g.g, 0)
	var perBlock, total C.int
	if rc := C.tdoa_num_stacks(m, C.int(windowsPerStack), &perBlock, &total); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_num_stacks: %s", C.GoString(C.tdoa_strerror(rc)))
	}
	pairs, stations := int(C.tdoa_num_pairs(m)), len(refDelay)
	if int(total)*pairs == 0 || stations*(stations-1)/2 != pairs || (mix != nil && len(mix) != int(total)) {
		return nil, fmt.Errorf("tdoa_group_process_sync_drift_locate: no stacks, fewer than two stations, not one delay per station or not one mix entry per stack")
	}
	o := newSyncDriftLocate(int(total), int(perBlock), stations, pairs)
	f, l := &o.SyncLinesFine, &o.LocateTrackZoom
	if rc := C.tdoa_group_process_sync_drift_locate(g.g, C.int(windowsPerStack), C.int(gate), C.int(maxDrift), C.int(driftDen), C.int(rounds),
		C.int(u), C.int(fineRounds), tablePtr(refDelay), centrePtr(centre), lineMixPtr(mix), C.int(maxStep), C.int(minSeparation), C.int(z),
		C.int(h), C.int(fineStep), C.int(fineSeparation), &f.Line[0], i32Ptr(f.Clock), i32Ptr(f.Rate), i32Ptr(f.Rows), i32Ptr(f.Lags),
		(*C.double)(unsafe.Pointer(&f.Corr[0])), &f.Fine[0], i32Ptr(f.Clock16), i32Ptr(f.FineRate), i32Ptr(f.FineRows), i32Ptr(f.FineLags),
		(*C.double)(unsafe.Pointer(&f.FineCorr[0])), i32Ptr(o.MixRows), &l.Track[0], i32Ptr(l.Cells), (*C.int64_t)(unsafe.Pointer(&l.Own[0])),
		i32Ptr(l.Lags), (*C.double)(unsafe.Pointer(&l.Corr[0])), nil, &l.ZTrack[0], i32Ptr(l.ZCells), (*C.int64_t)(unsafe.Pointer(&l.ZOwn[0])),
		i32Ptr(l.ZLags), (*C.double)(unsafe.Pointer(&l.ZCorr[0])), nil, nil); rc != C.TDOA_OK {
		return nil, fmt.Errorf("tdoa_group_process_sync_drift_locate: %s", C.GoString(C.tdoa_group_last_error(g.g)))
	}
	return o, nil
}
