// eh_host_selftest.h - host: self-test hooks of device primitives (byte movers, deflate / inflate) and of sort_by_priority.
#pragma once
// Self test hook: runs `njobs` byte-mover jobs ({kind,dst,src,n,plen} x uint32) on a caller
// supplied buffer image; jobs must touch disjoint destination ranges.  Returns the buffer.
int eh_selftest_movers(eh_ctx* ctx, uint8_t* buf, uint64_t buf_len, const uint32_t* jobs, uint32_t njobs, uint32_t* eq_out) {
  if (!ctx || !buf || !jobs) return EH_E_INVALID;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  DevBuf<uint8_t> d_buf; DevBuf<uint32_t> d_jobs, d_eq;
  hipError_t e = d_buf.grow(buf_len);
  if (e == hipSuccess) e = d_jobs.grow(5 * (uint64_t)njobs);
  if (e == hipSuccess) e = d_eq.grow(njobs);
  uint8_t* d = d_buf; uint32_t* dj = d_jobs; uint32_t* de = d_eq;
  if (e == hipSuccess) e = hipMemcpy(d, buf, buf_len, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dj, jobs, njobs * 20, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(de, 0, njobs * 4);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(eh_test_copy_kernel, dim3(njobs < 256 ? njobs : 256), dim3(64), 0, 0, d, dj, njobs, de);
    e = hipDeviceSynchronize();
  }
  if (e == hipSuccess) e = hipMemcpy(buf, d, buf_len, hipMemcpyDeviceToHost);
  if (e == hipSuccess && eq_out) e = hipMemcpy(eq_out, de, njobs * 4, hipMemcpyDeviceToHost);
  HIPCHK(ctx, e);
  return EH_OK;
}
// Self test hook for the device deflate / inflate (eh_zlib.h): op 0 raw deflate, 1 zlib:gzip/1, 2 zlib:deflate(default), 4 zlib:gunzip/1,
// 5 zlib:inflate/2 as mutate_once_compressed/6 uses it.  *ok = 0 where the reference's call raises.
int eh_selftest_zlib(eh_ctx* ctx, int op, const uint8_t* in, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* out_len, int32_t* ok) {
  if (!ctx || (!in && n) || !out || !out_len || !ok || op < 0 || op > 5 || op == 3 || (op <= 2 && cap < 64)) return EH_E_INVALID;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  DevBuf<uint8_t> d_in, d_out, d_scratch; DevBuf<uint64_t> d_res;
  hipError_t e = d_in.grow(n + 16);
  if (e == hipSuccess) e = d_out.grow(cap + 16);
  if (e == hipSuccess) e = d_scratch.grow(sizeof(ZDef) > sizeof(ZInf) ? sizeof(ZDef) : sizeof(ZInf));
  if (e == hipSuccess) e = d_res.grow(2);
  uint8_t* di = d_in; uint8_t* dout = d_out; uint8_t* ds = d_scratch; uint64_t* dr = d_res;
  if (e == hipSuccess && n) e = hipMemcpy(di, in, n, hipMemcpyHostToDevice);
  uint64_t r[2] = {0, 0};
  if (e == hipSuccess) {
    hipLaunchKernelGGL(eh_test_zlib_kernel, dim3(1), dim3(64), 0, 0, op, (const uint8_t*)di, n, dout, cap, ds, dr);
    e = hipDeviceSynchronize();
  }
  if (e == hipSuccess) e = hipMemcpy(r, dr, 16, hipMemcpyDeviceToHost);
  if (e == hipSuccess && r[1] && r[0] <= cap && r[0]) e = hipMemcpy(out, dout, r[0], hipMemcpyDeviceToHost);
  HIPCHK(ctx, e);
  *out_len = r[0]; *ok = (int32_t)r[1];
  return EH_OK;
}
int eh_selftest_sort_by_priority(const uint32_t* pri, uint32_t n, uint32_t* perm) {
  if ((!pri || !perm) && n) return EH_E_INVALID;
  PL in;
  for (uint32_t i = 0; i < n; i++) in.push_back(PItem{pri[i], (int)i});
  PL out = otp_sort_desc_strict(in);
  for (uint32_t i = 0; i < n; i++) perm[i] = (uint32_t)out[i].id;
  return EH_OK;
}
