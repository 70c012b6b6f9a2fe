/*
 * Drop-in replacement of the reference's public class (bao_flow_patchmatch_multiscale_cuda.h:33-44),
 * implemented on the MI355X-native C ABI of include/eppm.h.  Public names, signatures and argument
 * meaning are the reference's; the private section (CUDA vector-type buffer tables, :46-98 there) is
 * replaced by one opaque handle.
 *
 * Memory layout expected from the caller (basic/bao_basic.h:105-174): img[y][x][c] row-pointer tables
 * over R,G,B bytes, disp[y][x] row-pointer tables over floats; rows need not be contiguous.
 *
 * Differences from the reference, all on the error path: nothing here calls exit() or getchar();
 * a failed call prints one line to stderr and leaves the outputs untouched; init() may be called
 * again (the previous buffers are released first; the reference leaks them).
 */
#ifndef _BAO_FLOW_PATCHMATCH_MULTISCALE_CUDA_H_
#define _BAO_FLOW_PATCHMATCH_MULTISCALE_CUDA_H_

#include <stddef.h>
#include "bao_basic_cuda.h"   /* as the reference's header does (:31): callers get bao_timer_gpu / bao_timer_gpu_cpu through it */

struct eppm_ctx;
struct eppm_tracker;
struct eppm_track_params;

class bao_flow_patchmatch_multiscale_cuda
{
public:
    bao_flow_patchmatch_multiscale_cuda();
    ~bao_flow_patchmatch_multiscale_cuda();

public:
    //interface (bao_flow_patchmatch_multiscale_cuda.h:40-44)
    void init(int h,int w);
    void init(unsigned char***img1,unsigned char***img2,int h,int w);
    bool set_data(unsigned char***img1,unsigned char***img2); //always true in the reference (driver .cpp:159-168); false here only on error
    void compute_flow(float**disp1_x,float**disp1_y,unsigned char***color_flow=NULL);

    // additions (not in the reference): device selection and run-time values of the defs.h constants, both
    // before init(); access to the C handle
    void set_device(int device) { m_device = device; }
    // name = a field of eppm_params (include/eppm.h): "patch_r", "num_iter", "search_range", "num_guess",
    // "seg_len", "wmf_iters", "seed", "propagation", "levels"; or "pin_caller_buffers" (0/1, default 0): register the contiguous
    // image and flow blocks passed to set_data / compute_flow for DMA (eppm_host_register) the first time they are seen, so that no
    // host copy remains between the caller's memory and the GPU -- the caller then keeps those blocks allocated until the object
    // is destroyed or init() is called again.  false: unknown name.
    bool set_option(const char* name, long long value);
    eppm_ctx* handle() const { return m_ctx; }
    // compute_flow plus the backward flow (image 2 -> image 1) and the forward-backward occlusion masks (eppm_compute_bidirectional):
    // disp1_x, disp1_y receive what compute_flow writes, disp2_x, disp2_y the backward flow (the demo's disp2_x / disp2_y, main.cpp:46-51),
    // occ1 / occ2 (optional, h row pointers to w bytes) the masks of image 1's / image 2's pixels: 0 consistent, 1 inconsistent, 2 leaves
    // the frame, 3 unknown vector.  Same row-pointer tables, contiguous-block and pin_caller_buffers handling as compute_flow.
    void compute_flow_bidirectional(float** disp1_x, float** disp1_y, float** disp2_x, float** disp2_y, unsigned char** occ1 = NULL,
                                    unsigned char** occ2 = NULL);
    // alpha, beta of the masks' criterion (eppm_set_occlusion_params; defaults 0.01, 0.5); after init().  false: bad values or no context
    bool set_occlusion_params(float alpha, float beta);
    // draft mode (eppm_set_stop_level): the levels below `level` are upsampled edge-aware instead of refined; 0
    // (default) = the full path.  After init(); holds until the next init().  false: level outside 0 .. levels - 1 or no context
    bool set_stop_level(int level);
    // the frame at time t in [0, 1] between image 1 (t = 0) and image 2 (t = 1) (eppm_interpolate): valid after
    // compute_flow_bidirectional and until the next set_data; img_t: h x w x 3 R,G,B row-pointer tables (bao_alloc<unsigned char>(h, w, 3),
    // the layout of init's images).  false: no such call yet, bad t, or no context
    bool interpolate_frame(float t, unsigned char*** img_t);
    // dense point trajectories (eppm_tracker*): a tracker on this object's context (p NULL: the defaults; NULL: no
    // context or bad parameters), which the caller destroys (eppm_tracker_destroy) before init() or the destructor; track_step advances it
    // by the pair of the last compute_flow_bidirectional (eppm_track_step; false outside that window); the tracks: eppm_tracker_get
    eppm_tracker* create_tracker(const eppm_track_params* p = NULL);
    bool track_step(eppm_tracker* t);

private:
    void _destroy();

private:
    int m_h;
    int m_w;
    int m_device;
    eppm_ctx* m_ctx;
    void* m_params;           // eppm_params*
    unsigned char* m_stage;   // contiguous RGB staging for row-pointer inputs that are not one block (allocated when needed)
    float* m_u;               // ... and for flow planes whose rows are not contiguous
    float* m_v;
    void* m_priv;             // caller blocks seen so far (verified layouts, DMA registrations)
};

#endif
